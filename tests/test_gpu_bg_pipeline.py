"""The background-tile pipeline of a registration batch (detect.hip: ab_bg_pipeline_*) at its chunk boundaries, against the calls that
do not use it.  No oracle here: a batch must equal the single-pair calls (which estimate each frame's background in the frame's own
chain) exactly, and the host-fed form (percentiles per chunk, a feeder thread, chunks of four planes) must equal the device-resident
one (percentiles up front, a first launch of five planes, then sixteen per launch) bit for bit.  A plane whose worker waited for the
wrong launch's event, or read another plane's tiles, shows as a different transform.

n targets put n + 1 planes (the reference first) through the pipeline: 5, 6, 21 and 22 planes are the first launch's boundary and the
16-plane launch's boundary +- 1, and for the fed form multiples of four +- 1.  Three targets are registered without a pipeline.
(300, 403): ragged 37-px tiles, no candidate lists.  (2048, 2048): 256-px tiles, candidate lists for the labelling pass.
"""
import dataclasses

import pytest

pytestmark = pytest.mark.gpu

COUNTS = (3, 4, 5, 20, 21)


def _fields(r):
    return (r.method, r.matched_stars, r.inliers, r.transform, r.residual_px)


def _frames(rows, cols, n_stars, n_targets, device):
    from astroburst_amd import synth
    y, x, flux = synth.star_catalog(rows, cols, n_stars, seed=rows)
    cat = (y, x, flux * 30.0)
    ref = synth.make_frame(rows, cols, 0, cat=cat, device=device, bad_patch_rate=0.0, cosmic_rate=1e-4)
    tgts = [synth.make_frame(rows, cols, k + 1, cat=cat, device=device, shift=(0.45 * k - 4.5, 3.75 - 0.35 * k), bad_patch_rate=1e-6, cosmic_rate=1e-4)
            for k in range(n_targets)]
    return ref, tgts


@pytest.fixture(scope="module")
def small(ctx):
    """one reference and 21 targets of (300, 403) on the device, their host copies, and the single-pair result of every target"""
    ref, tgts = _frames(300, 403, 260, 21, "cpu")
    singles = [ctx.align_channel_affine(ref.numpy(), t.numpy(), num_threads=8) for t in tgts]
    # the premise: every pair registers on its stars (a pair that fell back to phase correlation would not have used the pipeline's tiles)
    assert all(s.method in ("affine", "rigid") for s in singles), [s.method for s in singles]
    return ref.cuda(), [t.cuda() for t in tgts], [t.numpy() for t in tgts], singles


def _fed_equals_resident(ctx, ref, dev, host):
    import torch
    want_out = [torch.full_like(d, -1.0) for d in dev]
    want = ctx.align_pairs_affine(ref, dev, want_out, num_threads=8)
    got_out = [torch.full_like(d, -2.0) for d in dev]
    got = ctx.align_pairs_affine(ref, host, got_out, num_threads=8)
    for k, (g, w, o, wo) in enumerate(zip(got, want, got_out, want_out)):
        assert (g.method, g.transform, g.inliers, g.matched_stars) == (w.method, w.transform, w.inliers, w.matched_stars), k
        assert torch.equal(o.isnan(), wo.isnan()) and torch.equal(o.nan_to_num(), wo.nan_to_num()), k
    return want


@pytest.mark.parametrize("n", COUNTS)
def test_batches_at_the_chunk_boundaries(ctx, small, n):
    ref, dev, host, singles = small
    before = ctx.fallback_counts()
    batch = ctx.register_frames(ref, dev[:n], num_threads=8)
    assert len(batch) == n
    for k, (b, s) in enumerate(zip(batch, singles)):
        assert _fields(b) == _fields(s), (n, k)
    resident = _fed_equals_resident(ctx, ref, dev[:n], host[:n])
    assert [_fields(r) for r in resident] == [_fields(b) for b in batch]
    assert ctx.fallback_counts()["frames_redone"] == before["frames_redone"], "an ordinary star field must not need the full path"


def test_candidate_lists_and_a_short_first_launch(ctx):
    """(2048, 2048): six planes = a first launch of five and a launch of one, whose tiles also leave the labelling pass's candidate lists"""
    ref, dev = _frames(2048, 2048, 3900, 5, "cuda")
    host = [t.cpu().numpy() for t in dev]
    resident = _fed_equals_resident(ctx, ref, dev, host)
    batch = ctx.register_frames(ref, dev, num_threads=8)
    assert [_fields(b) for b in batch] == [_fields(r) for r in resident]
    ref_h = ref.cpu().numpy()
    for k in (0, 4):   # one target of each launch
        single = ctx.align_channel_affine(ref_h, host[k], num_threads=8)
        assert single.method in ("affine", "rigid")
        assert _fields(batch[k]) == _fields(single), k


def test_nine_uniform_subframes_equal_the_single_calls(ctx, small):
    """analyze_subframes of nine device frames of one size takes their backgrounds from the pipeline (launches of five and four planes);
    one frame at a time estimates its own"""
    _, dev, _, _ = small
    got = ctx.analyze_subframes(dev[:9])
    assert len(got) == 9 and any(g.star_count > 0 for g in got)
    for k, (g, d) in enumerate(zip(got, dev[:9])):
        one = ctx.analyze_subframe(d)
        for f in dataclasses.fields(g):   # field for field; a NaN (no stars, no FWHM) equals a NaN
            a, b = getattr(g, f.name), getattr(one, f.name)
            assert a == b or (a != a and b != b), (k, f.name, a, b)
