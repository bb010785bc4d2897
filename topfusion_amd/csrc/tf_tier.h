// tf_tier.h -- what a hash entry of a swapping scene holds across its two tiers (the VBA and the GlobalCache),
// written once (DESIGN.md §Mesh extraction, the whole map): the mesher's whole reading (tf_mesh_dev.h), the free
// views' whole reading (tf_render.hip, tf_view.hip) and every later reader of both tiers take the rule from here.
// The voxel of a block whose merge is pending is tf_swap_combine.h's sw_combine(stored, active, maxW).
//
// A scene type S of the whole reading has: v (SceneView), state (HashSwapState::state per entry), flags
// (hasStoredData per entry), store (storedVoxelBlocks: 512 voxels per entry) and maxW.
#pragma once
#include "tf_internal.h"
#include "tf_swap_combine.h"

// A resolved block: where its voxels lie.  act = the VBA voxel offset (ptr * 512) or TF_VOFF_NONE, sto = the
// GlobalCache voxel offset (entry * 512; tf_create bounds the table so it fits an int) or TIER_STO_NONE.
// Both: the voxel is CombineVoxelInformation(stored, active); neither: the block is missing.  ent = the hash
// entry the block was found at (-1: missing) -- what the indexed mesh keys a block's edge bits by.
#define TIER_STO_NONE (-1)
struct TierBlk {
    int act, sto, ent;
};

// Entry ei with the block pointer ptr, by the table: a block and no store, or a store left behind by a
// finished merge (state 2: k_swap_in never clears the flag) -> the active block; a block and a store not
// yet merged -> both; swapped out with a store -> the store; anything else is missing.
template <class S>
__device__ __forceinline__ TierBlk tier_resolve_entry(const S& s, int ei, int ptr)
{
    const bool stored = s.flags[ei] != 0;
    TierBlk d = { TF_VOFF_NONE, TIER_STO_NONE, -1 };
    if (ptr >= 0) {
        d.act = ptr * TF_BLK3;
        d.ent = ei;
        if (stored && s.state[ei] != 2) d.sto = ei * TF_BLK3;
    } else if (ptr == -1 && stored) {
        d.sto = ei * TF_BLK3;
        d.ent = ei;
    }
    return d;
}

// does an entry with the block pointer ptr hold voxel data in either tier; flags is read only where ptr == -1
__device__ __forceinline__ bool tier_ptr_resolves(const unsigned char* flags, int idx, int ptr)
{
    return ptr >= 0 || (ptr == -1 && flags[idx] != 0);
}
template <class S>
__device__ __forceinline__ bool tier_entry_resolves(const S& s, int idx)
{
    return tier_ptr_resolves(s.flags, idx, s.v.hash[idx].ptr);
}

// blk_walk over both tiers: the first entry at the block that resolves (ptr >= 0, or swapped out -- ptr -1 --
// with stored data), or -1
template <class S>
__device__ __forceinline__ int tier_walk(const S& s, int bx, int by, int bz)
{
    int hi = tf_hash_index(bx, by, bz, s.v.mask);
    while (true) {
        const TfHashEntry e = s.v.hash[hi];
        if (e.x == (short)bx && e.y == (short)by && e.z == (short)bz && tier_ptr_resolves(s.flags, hi, e.ptr)) return hi;
        if (e.offset < 1) return -1;
        hi = s.v.n_buckets + e.offset - 1;
    }
}

// The block at a position over both tiers.  The block grid first: a hit is a block in the VBA, whose entry's flag
// and state say whether a merge is pending.  A miss inside the grid is not the end -- swap-out clears the cell, so a
// stored block is never in the grid -- and takes the hash walk, as a block outside the grid does.  (tier_walk
// compares the coordinates as shorts: a caller that can leave their range checks it first.)
template <class S>
__device__ __forceinline__ TierBlk tier_block_find(const S& s, int bx, int by, int bz)
{
    if (tf_grid_in(bx, by, bz)) {
        const int2 b = s.v.grid[tf_grid_cell(bx, by, bz)];
        if (b.x >= 0) return tier_resolve_entry(s, b.x, b.y >> 9);
    }
    const TierBlk none = { TF_VOFF_NONE, TIER_STO_NONE, -1 };
    const int hi = tier_walk(s, bx, by, bz);
    return hi < 0 ? none : tier_resolve_entry(s, hi, s.v.hash[hi].ptr);
}
