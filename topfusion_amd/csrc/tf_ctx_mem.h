// tf_ctx_mem.h -- the one owner of a context's device and pinned memory.  Host only, no HIP header: the
// allocate / free functions come in as pointers at construction (tf_capi.hip hands in HIP's; tests/ctx_mem_main.cpp
// a counting malloc that fails on its k-th call).  The registry records the pointer VALUES it hands out, not
// where the caller keeps them, so pointers may be exchanged among members (swap_pyramids, the fused batch's
// two dists buffers).  Three operations: one buffer, a group all or none, one buffer released early;
// destruction frees what is still recorded.  A scoped temporary is a local TfCtxMem of the same functions.
// Beside it TfCtxViews: the free views (tf_view.hip) alive on a context, so that the context can drop the host
// part of those its caller never destroyed (their buffers are the registry's like any other).
#pragma once
#include <stddef.h>
#include <initializer_list>
#include <new>
#include <vector>

// 0 is success; every other value is the allocator's own error code and is returned unchanged
struct TfMemFns {
    int (*dev_alloc)(void** p, size_t bytes);
    int (*dev_free)(void* p);
    int (*pin_alloc)(void** p, size_t bytes, unsigned flags);
    int (*pin_free)(void* p);
    int oom;                 // the code for "the registry's own record could not grow"
};

class TfCtxMem {
public:
    // one buffer of a group: device memory, or pinned host memory with the allocator's flags
    struct Req {
        void** p;
        size_t bytes;
        bool pinned;
        unsigned flags;
    };
    template <class T> static Req dev(T** p, size_t bytes) { return Req{ (void**)p, bytes, false, 0u }; }
    template <class T> static Req pin(T** p, size_t bytes, unsigned flags) { return Req{ (void**)p, bytes, true, flags }; }

    explicit TfCtxMem(const TfMemFns& f) : fns_(f) {}
    TfCtxMem(const TfCtxMem&) = delete;
    TfCtxMem& operator=(const TfCtxMem&) = delete;
    ~TfCtxMem()
    {
        for (size_t i = recs_.size(); i-- > 0;) free_rec(recs_[i]);
    }
    const TfMemFns& fns() const { return fns_; }

    // one buffer into *p (nullptr on failure); device buffers are 16 bytes at least
    int alloc(const Req& r)
    {
        *r.p = nullptr;
        try { recs_.push_back(Rec{ nullptr, r.pinned }); } catch (const std::bad_alloc&) { return fns_.oom; }
        void* q = nullptr;
        const int e = r.pinned ? fns_.pin_alloc(&q, r.bytes, r.flags) : fns_.dev_alloc(&q, r.bytes < 16 ? 16 : r.bytes);
        if (e != 0 || !q) { recs_.pop_back(); return e; }
        recs_.back().p = q;
        *r.p = q;
        return 0;
    }
    template <class T> int alloc(T** p, size_t bytes) { return alloc(dev(p, bytes)); }

    // a group, all or none: on a failure what the group already got is freed, all its pointers are null
    int alloc_group(std::initializer_list<Req> group)
    {
        int e = 0;
        for (const Req& r : group) *r.p = nullptr;
        for (const Req& r : group)
            if ((e = alloc(r)) != 0) break;
        if (e != 0)
            for (const Req& r : group) (void)release(*r.p);
        return e;
    }

    // one buffer back before the owner goes (nullptr: nothing); p is null afterwards
    template <class T> int release(T*& p)
    {
        int e = 0;
        for (size_t i = recs_.size(); p && i-- > 0;)
            if (recs_[i].p == (void*)p) {
                e = free_rec(recs_[i]);
                recs_.erase(recs_.begin() + (ptrdiff_t)i);
                break;
            }
        p = nullptr;
        return e;
    }

private:
    struct Rec {
        void* p;
        bool pinned;
    };
    int free_rec(const Rec& r) { return r.pinned ? fns_.pin_free(r.p) : fns_.dev_free(r.p); }
    TfMemFns fns_;
    std::vector<Rec> recs_;
};

// The free views alive on a context.  A view's buffers come from the context's TfCtxMem; this records the host
// objects: add at tf_view_create, remove at tf_view_destroy (false: not a live view of this context, nothing
// to destroy), and at destruction `drop` for each one still recorded, newest first.  Declared after the
// TfCtxMem in tf_ctx, so it goes first.
class TfCtxViews {
public:
    typedef void (*Drop)(void* view);
    TfCtxViews() {}
    TfCtxViews(const TfCtxViews&) = delete;
    TfCtxViews& operator=(const TfCtxViews&) = delete;
    ~TfCtxViews()
    {
        for (size_t i = recs_.size(); i-- > 0;) recs_[i].drop(recs_[i].view);
    }
    // 0, or `oom` when the record could not grow (the view is then not recorded)
    int add(void* view, Drop drop, int oom)
    {
        try { recs_.push_back(Rec{ view, drop }); } catch (const std::bad_alloc&) { return oom; }
        return 0;
    }
    bool remove(const void* view)
    {
        for (size_t i = recs_.size(); view && i-- > 0;)
            if (recs_[i].view == view) {
                recs_.erase(recs_.begin() + (ptrdiff_t)i);
                return true;
            }
        return false;
    }
    bool live(const void* view) const
    {
        for (const Rec& r : recs_) if (r.view == view) return true;
        return false;
    }
    size_t count() const { return recs_.size(); }

private:
    struct Rec {
        void* view;
        Drop drop;
    };
    std::vector<Rec> recs_;
};
