"""AllocateSceneFromDepth on constructed depth images and tables (tests/alloc_cases.py) against the oracle's tfo_alloc_ex,
bit for bit after every call: the hash (every field), the visible types, the visible ids up to noVisibleEntries, the
three counters, the call's failure counts, both free lists and, on a swapping context, the swap states and the
re-allocation count.  No tolerances.  The inputs sit on the index edges of k_alloc_requests, k_alloc_apply,
k_alloc_discard, k_set_type3, k_vis_build / k_vis_count + k_vis_apply and the swapping re-allocation in
topfusion_amd/csrc/tf_scene.hip; tests/test_alloc_cases.py asserts on the CPU that each family reaches its edge and
that a plain restatement of the reference's definition agrees with the oracle on all of them.

  slots     255 | 256 | 257 and 600+ distinct entries requested by one 16 x 16 tile (AllocLds, its `seen` table on the
            runs that find them again), an entry requested through one tile's table and straight to memory by another
  steps     1, 2, 3, 8, 9, 16, 17 and 58 steps per pixel: later batches of 8, step indices up to 57 in the winner key
  collide   256 buckets: frame after frame until the chains hold every block
  grid      segments across block coordinates -129 | -128 and 127 | 128 of each axis, over tables holding blocks on both
            sides in the bucket, deep in a chain and swapped out; a request at the table's last entry
  skip      both sides of every rejection test of the depth value
  apply     counters set to the exact fits and the exhaustion orders of the serial allocation loop, permuted free
            lists, chunks with more than 512 requests, with none, ragged
  vis       the tracker's visible-list cap below, at and above the need (one past a chunk), fused and in two launches
  swapping  the grid and apply tables on a swapping context: the blocks run out halfway through the re-allocations

Every family's first case also runs with onlyUpdateVisibleList, with resetVisibleList and under a rotated pose, and is
followed by tf_scene_integrate and a raycast (VBA and raycast result compared: the block grid still mirrors the hash).
What mutations of the kernels these catch: profiles/alloc_edges_mutation_check.txt."""
import numpy as np
import pytest

import alloc_cases as A
from parity_util import assert_bit_exact, assert_struct_exact
from test_alloc_cases import HASH_FIELDS, load_oracle

pytestmark = pytest.mark.gpu


class Side:
    """A GPU context and an oracle of one parameter set, driven in step."""

    def __init__(self, O, kw, env):
        from topfusion_amd import TopFu, _lib, default_params
        from test_gpu_engines import Pitched
        self.L, self.O, self.kw = _lib, O, kw
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            self.g = TopFu(default_params(**kw))
        self.o = O.Oracle(O.default_params(**kw))
        self.intr = np.array([kw[k] for k in ("fx", "fy", "cx", "cy")], np.float32)
        self.dists = Pitched(kw["rows"], kw["cols"], np.float32)
        self.swapping = bool(kw["use_swapping"])

    def load(self, s):
        g, L = self.g, self.L
        g.upload(L.TF_BUF_HASH, s["hash"])
        g.upload(L.TF_BUF_VISIBLE_TYPE, s["vis_type"])
        g.upload(L.TF_BUF_VISIBLE_IDS, s["visible_ids"])
        g.upload(L.TF_BUF_ALLOC_LIST, s["alloc_list"])
        g.upload(L.TF_BUF_EXCESS_LIST, s["excess_list"])
        if self.swapping:
            g.upload(L.TF_BUF_SWAP_STATE, s["swap_state"])
            g.upload(L.TF_BUF_SWAP_STORED_FLAGS, (s["hash"]["ptr"] == -1).astype(np.uint8))
        g.set_counters(*s["counters"])
        load_oracle(self.o, s)
        return self

    def alloc(self, tag, pose, dists, only, reset):
        from test_gpu_engines import _f, _ok
        before = self.g.totals()
        self.dists.put(dists)
        _ok(self.L.load().tf_scene_alloc(self.g._h, _f(self.intr), _f(pose), self.dists.ptr, self.dists.step, int(only), int(reset)),
            "tf_scene_alloc")
        self.o.alloc(pose, dists, only_update_visible=only, reset_visible=reset)
        after = self.g.totals()
        self.compare(tag, tuple(int(after[k] - before[k]) for k in ("alloc_failed_type1", "alloc_failed_type2")))

    def compare(self, tag, failed):
        g, o = self.g, self.o
        assert_struct_exact(f"{tag} hash", g.hash(), o.hash(), HASH_FIELDS)
        assert_bit_exact(f"{tag} visible types", g.visible_type(), o.visible_type())
        sg, so = g.stats(), o.counters()
        for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries"):
            assert sg[k] == so[k], f"{tag} {k}: gpu {sg[k]} oracle {so[k]}"
        assert_bit_exact(f"{tag} visible ids", g.visible_ids(), o.visible_ids())
        assert failed == o.alloc_failures(), f"{tag} failed requests: gpu {failed} oracle {o.alloc_failures()}"
        assert_bit_exact(f"{tag} free blocks", g.alloc_list(), o.alloc_list())
        assert_bit_exact(f"{tag} free excess entries", g.excess_list(), o.excess_list())
        if self.swapping:
            assert_bit_exact(f"{tag} swap states", g.swap_state(), o.swap_state())
            assert g.swap_counts()[2] == o.swap_counts()[2], f"{tag} re-allocated: gpu {g.swap_counts()} oracle {o.swap_counts()}"

    def integrate_and_raycast(self, tag, pose, dists):
        """IntegrateIntoScene over the visible list, then CreateExpectedDepths and a raycast: both read blocks through
        the hash's mirror, the block grid, which the allocation kept."""
        from test_gpu_engines import _f, _ok
        self.dists.put(dists)
        _ok(self.L.load().tf_scene_integrate(self.g._h, _f(self.intr), _f(pose), self.dists.ptr, self.dists.step), "tf_scene_integrate")
        self.o.integrate(pose, dists)
        assert_struct_exact(f"{tag} vba", self.g.vba(), self.o.vba(), ["sdf", "w"])
        c2w = self.O.rigid_inv(pose)
        self.g.stage_expected_depths(pose)
        self.o.expected_depths(pose)
        self.g.stage_raycast(c2w, 1)
        self.o.raycast(c2w, 1)
        assert_bit_exact(f"{tag} raycast", self.g.raycast_result(), self.o.raycast_result())
        assert_bit_exact(f"{tag} visible types after the raycast", self.g.visible_type(), self.o.visible_type())
        assert (self.o.vba()["w"] > 0).any(), f"{tag}: nothing integrated"

    def close(self):
        self.dists.free()
        self.g.close()


def _family(c):
    return next(f for f in A.FAMILIES if c.name.startswith(f))


@pytest.fixture(scope="module")
def sides(oracle_mod):
    """Contexts shared per parameter set and creation environment, one family's at a time."""
    made, family = {}, [None]

    def close_all():
        for side in made.values():
            side.close()
        made.clear()

    def get(c):
        if family[0] != _family(c):
            close_all()
            family[0] = _family(c)
        key = (tuple(sorted(c.kw.items())), tuple(sorted(c.env.items())))
        if key not in made:
            made[key] = Side(oracle_mod, c.kw, c.env)
        return made[key]

    yield get
    close_all()


FIRST = {f()[0].name for f in A.FAMILIES.values()}


@pytest.mark.parametrize("c", A.all_cases(), ids=lambda c: c.name)
def test_case(sides, c):
    side = sides(c).load(c.state)
    for k, (pose, dists, only, reset) in enumerate(c.calls):
        side.alloc(f"{c.name} call {k}", pose, dists, only, reset)
    if c.name in FIRST:
        side.integrate_and_raycast(c.name, *c.calls[-1][:2])


def test_mu_bound():
    """tf_create takes the largest mu / voxelSize ratio the steps family runs at and refuses the next float."""
    from topfusion_amd import TopFu, _lib, default_params
    lo, hi = A.mu_largest()
    TopFu(default_params(**A.params_kw(36, 28, mu=lo))).close()
    with pytest.raises(_lib.TfError) as e:
        TopFu(default_params(**A.params_kw(36, 28, mu=hi)))
    assert e.value.status == _lib.TF_INVALID_ARG
