"""The DEVICE triangle matcher (csrc/affine.hip: tri_build, tri_bin_scan, tri_scatter, tri_bucket_sort, tri_group_windows and the
vote kernels, each also as a *_many kernel for a group of frames) fed star lists directly through ab_triangle_votes_device -- the
functions register_one / register_group run, not copies -- and held to the restatement's vote matrix (tests/affine_restatement.py)
on the crafted lists of tests/triangle_cases.py, in every cell.  Votes are integers: no tolerance anywhere.  What each family is
for, and the proof that it still does it, is in tests/triangle_cases.py and tests/test_triangle_cases_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import triangle_cases as tc

pytestmark = pytest.mark.gpu

NAMES = list(tc.CASES)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, int(bad.shape[0]), [(int(r), int(t), int(got[r, t]), int(want[r, t])) for r, t in bad[:8]])


@pytest.mark.parametrize("grouped", [False, True], ids=["one by one", "grouped"])
@pytest.mark.parametrize("name", NAMES)
def test_device_votes_equal_the_restatement(ctx, name, grouped):
    ref, tgt = tc.CASES[name]
    assert_same(ctx.triangle_votes(ref, [tgt], grouped=grouped)[0], tc.want_case(name), name)


def group_targets(order):
    return tc.GROUP_TARGETS if order == "given" else tc.GROUP_TARGETS[::-1]


@pytest.mark.parametrize("grouped", [False, True], ids=["one by one", "grouped"])
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_neighbours_and_position_in_a_group_do_not_matter(ctx, order, grouped):
    """eleven targets -- groups of 8 + 3 -- among them an empty list, a 3-star list and a cluster without a surviving triangle (each
    still owns its blockIdx.y): every matrix equals the target's stand-alone one, the device's and the restatement's"""
    targets = group_targets(order)
    got = ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped)
    assert got.shape == (11, 64, 64)
    for k, t in enumerate(targets):
        assert_same(got[k], tc.want(tc.GROUP_REF, t), (order, k))
        assert_same(got[k], ctx.triangle_votes(tc.GROUP_REF, [t], grouped=grouped)[0], (order, k, "alone"))


@pytest.mark.parametrize("grouped", [False, True], ids=["one by one", "grouped"])
def test_no_state_leaks_between_calls_nor_through_a_trim_nor_past_a_refusal(ctx, grouped):
    """The vote kernel resets the target table's counter, the scan re-zeroes the bucket histogram, a fresh workspace is zeroed by a
    memset: the same call twice gives the same matrices, so does the call after ab_ctx_trim released the workspaces, and so does
    the call after one that was refused (a NaN coordinate)."""
    import astroburst_amd as ab
    targets = group_targets("given")
    first = ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped)
    for k, t in enumerate(targets):
        assert_same(first[k], tc.want(tc.GROUP_REF, t), k)
    assert np.array_equal(ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped), first)
    # another reference in between: the reference table and its group windows are rebuilt per call
    assert_same(ctx.triangle_votes(tc.LATTICE_3X3, [tc.LATTICE_3X3], grouped=grouped)[0], tc.want_case("E lattice 3x3"), "3x3 in between")
    assert np.array_equal(ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped), first)
    ctx.trim()
    assert np.array_equal(ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped), first)
    broken = [t.copy() for t in targets]
    broken[8][3, 1] = np.nan
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.triangle_votes(tc.GROUP_REF, broken, grouped=grouped)
    assert e.value.code == ab._lib.AB_ERR_INVALID
    bad_ref = tc.GROUP_REF.copy()
    bad_ref[59, 0] = np.inf
    with pytest.raises(ab.AstroBurstError):
        ctx.triangle_votes(bad_ref, targets, grouped=grouped)
    assert np.array_equal(ctx.triangle_votes(tc.GROUP_REF, targets, grouped=grouped), first)


def test_a_short_reference_list_and_no_targets(ctx):
    got = ctx.triangle_votes(tc.n_list(3), group_targets("given"), grouped=True)
    assert got.shape == (11, 64, 64) and not got.any()
    assert not ctx.triangle_votes(tc.n_list(3), group_targets("given")).any()
    assert ctx.triangle_votes(tc.GROUP_REF, []).shape == (0, 64, 64)


# ---- the superseded forms of the vote kernel (developer library) ----------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import astroburst_amd as ab
import triangle_cases as tc
ctx = ab.Context(0)
out = {}
names = [n for n in tc.CASES if n[0] in "EBT"]
for g in (False, True):
    for i, n in enumerate(names):
        out["case %%d %%d" %% (i, g)] = ctx.triangle_votes(tc.CASES[n][0], [tc.CASES[n][1]], grouped=g)[0]
    out["group given %%d" %% g] = ctx.triangle_votes(tc.GROUP_REF, tc.GROUP_TARGETS, grouped=g)
    out["group reversed %%d" %% g] = ctx.triangle_votes(tc.GROUP_REF, tc.GROUP_TARGETS[::-1], grouped=g)
ctx.close()
np.savez(%(out)r, **out)
print("DONE", len(out))
"""

FORMS = [{"AB_VOTE_WAVES": "1"}, {"AB_VOTE_SLICES": "1"}, {"AB_VOTE_SLICES": "3"}, {"AB_VOTE_COPIES": "1"}, {"AB_VOTE_COPIES": "16"}]


@pytest.mark.parametrize("form", FORMS, ids=["%s=%s" % kv for f in FORMS for kv in f.items()])
def test_superseded_vote_forms_equal_the_restatement(tmp_path, dev_build, form):
    """AB_VOTE_WAVES=1 (persistent one-wave blocks), AB_VOTE_SLICES (slices of a reference group's candidate range: 1 = none, 3 = a
    `per` that does not divide), AB_VOTE_COPIES (copies of the matrix the blocks flush into; 16 moves the switch between the
    builder's threads and the memset clearing them to 41 stars).  They are read once per process: a fresh child each, families E,
    B, T and G through both forms of the entry point, the matrices compared here."""
    out = tmp_path / "votes.npz"
    env = dict(os.environ)
    for k in ("AB_VOTE_WAVES", "AB_VOTE_SLICES", "AB_VOTE_COPIES"):
        env.pop(k, None)
    env.update(form)
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(out))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    names = [n for n in tc.CASES if n[0] in "EBT"]
    for g in (0, 1):
        for i, n in enumerate(names):
            assert_same(got["case %d %d" % (i, g)], tc.want_case(n), (form, n, g))
        for order in ("given", "reversed"):
            for k, t in enumerate(group_targets(order)):
                assert_same(got["group %s %d" % (order, g)][k], tc.want(tc.GROUP_REF, t), (form, order, k, g))
