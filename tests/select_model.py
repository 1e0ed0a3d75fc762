"""A numpy model of the HOST logic of csrc/plane_select.hip (ab_plane_select_ranks' descend / locate, ab_plane_order_stats,
ab_plane_median_f32, and percentile_bounds of csrc/render.hip), with the histogram kernel replaced by np.bincount.

It is no checker of the library: it exists so that tests/test_select_adversarial_cpu.py can show, without a GPU, that the fixtures of
tests/select_adversarial.py tell a subtly wrong select from a right one.  `mutation` switches one arithmetic mistake on:

  a  locate: `cum + h[i] >= rank` for `>`
  b  the rank of the low percentile is clamped nowhere, neither in percentile_bounds nor in the select.  (The select's own clamp is
     redundant today, because every caller clamps: a mutation that only moves the clamp into the caller is no mistake until the
     caller forgets one rank.  This is that state: the high rank is clamped by the caller, the low one -- which only the reversed
     pair (1, 0) pushes to `count` -- is not.)
  c  level 1 fills h1 with its child pass as well (no separate h2)
  d  the median of an even count is its upper middle value
  e  the key of use_dev is v - center, not |v - center|

  f  (masked_stretch_chain, the model of csrc/masked_stretch.hip's device-resident select) level 1 reads the blend pass's predicted
     histogram whenever a prediction was made, whether or not the level-0 pick found the predicted bin

Mutation c changes nothing, here or in the library: descend locates every item of a level in that level's histogram BEFORE its first
child pass, so the histogram is never read again once a child pass may overwrite it.
"""
import numpy as np

F32 = np.float32
SHIFTS, BITS = (21, 10, 0), (11, 11, 10)


def select_ranks(data, min_valid, use_dev, center, ranks_of, mutation=""):
    """-> (count, [value of ranks_of(count)[i]]); nothing is selected without a candidate"""
    v = np.asarray(data, F32).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        c = v[np.isfinite(v) & (v > F32(min_valid))]
        k = (c - F32(center)).astype(F32) if use_dev else c
        if use_dev and mutation != "e":
            k = np.abs(k)
    keys = np.ascontiguousarray(k, dtype=F32).view(np.uint32)

    def run_pass(mask, val, level):
        sel = keys[(keys & np.uint32(mask)) == np.uint32(val)]
        return np.bincount((sel >> np.uint32(SHIFTS[level])) & np.uint32((1 << BITS[level]) - 1), minlength=1 << BITS[level]).astype(np.int64)

    def locate(h, rank):
        cum = np.cumsum(h)
        hit = np.nonzero(cum >= rank if mutation == "a" else cum > rank)[0]
        if hit.size == 0:
            return h.size - 1, 0
        i = int(hit[0])
        return i, rank - int(cum[i] - h[i])

    buffers = {0: run_pass(0, 0, 0)}                 # 0: h0, 1: h1, 2: h2 -- overwritten in place like the pinned histograms
    count = int(buffers[0].sum())
    if count == 0:
        return 0, []
    ranks = list(ranks_of(count))
    vals = [None] * len(ranks)

    def descend(level, mask, val, slot, items):
        groups = []
        for r, rank in items:
            b, within = locate(buffers[slot], rank)
            if not groups or groups[-1][0] != b:
                groups.append((b, []))
            groups[-1][1].append((r, within))
        for b, its in groups:
            value = val | (b << SHIFTS[level])
            if level == 2:
                for r, _ in its:
                    vals[r] = np.array([value], np.uint32).view(F32)[0]
                continue
            m = mask | (((1 << BITS[level]) - 1) << SHIFTS[level])
            nxt = 1 if (level == 0 or mutation == "c") else 2
            buffers[nxt] = run_pass(m, value, level + 1)
            descend(level + 1, m, value, nxt, its)

    items = sorted(((r, rank if mutation == "b" else min(rank, count - 1)) for r, rank in enumerate(ranks)), key=lambda t: t[1])
    descend(0, 0, 0, 0, items)
    return count, vals


def percentile_bounds(data, low_pct, high_pct, mutation=""):
    """percentile_bounds of csrc/render.hip -> (lo, hi), or None where it takes the min / max branch"""
    def ranks_of(m):
        low = int(float(m) * low_pct)
        return [low if mutation == "b" else min(low, m - 1), min(int(float(m) * high_pct), m - 1)]
    count, vals = select_ranks(data, 1e-7, False, 0.0, ranks_of, mutation)
    return None if count == 0 else (vals[0], vals[1])


def median_f32(data, min_valid=0.0, use_dev=False, center=0.0, mutation=""):
    """ab_plane_median_f32"""
    count, vals = select_ranks(data, min_valid, use_dev, center, lambda c: [c // 2, c // 2 - 1] if c % 2 == 0 else [c // 2], mutation)
    if count == 0:
        return F32(0.0)
    if count % 2 or mutation == "d":
        return vals[0]
    return F32(F32(vals[1] + vals[0]) / F32(2.0))


# ---- the device-resident select of csrc/masked_stretch.hip, with its speculative level 1 ----------------------------------------
def masked_stretch_chain(image, mask, iterations=10, target_background=0.25, protection_amount=0.85, convergence_threshold=1e-5,
                         mutation="", predict=True):
    """masked_stretch_enqueue as a sequence of numpy steps: ms_pick_kernel's three levels per median, the loop's head, the blend
    that histograms level 0 of the next median and level 1 under the PREDICTED level-0 bin.  predict=False is AB_MS_NO_PREDICT.
    -> (image, iterations_run, final_background, converged, [(predicted bin, real bin)] per median after a blend)"""
    import masked_restatement as MR
    working = MR.normalize_to_01(image)
    mask = np.asarray(mask, F32)
    protection = F32(protection_amount)
    st = dict(pred_b0=0, pred_valid=False, pred_hist=np.zeros(2048, np.int64))
    trace = []

    def keys_of():
        with np.errstate(invalid="ignore"):
            sel = (mask < F32(0.5)) & np.isfinite(working) & (working > F32(0.0))
        return np.ascontiguousarray(working[sel]).view(np.uint32)

    def pick(h, rank):
        cum = np.cumsum(h)
        hit = np.nonzero(cum > rank)[0]
        if hit.size == 0:
            return h.size - 1, 0
        i = int(hit[0])
        return i, rank - int(cum[i] - h[i])

    def median():
        keys = keys_of()
        if keys.size == 0:
            st["pred_valid"] = False
            return 0.0
        b0, rank = pick(np.bincount(keys >> np.uint32(21), minlength=2048), keys.size // 2)
        if st["pred_valid"]:
            trace.append((st["pred_b0"], b0))
        l1_ready = st["pred_valid"] and b0 == st["pred_b0"]
        fresh = np.bincount((keys[(keys >> np.uint32(21)) == b0] >> np.uint32(10)) & np.uint32(0x7FF), minlength=2048)
        b1, rank = pick(st["pred_hist"] if (l1_ready or (mutation == "f" and st["pred_valid"])) else fresh, rank)
        st["pred_valid"] = False
        prefix = (b0 << 21) | (b1 << 10)
        b2, _ = pick(np.bincount(keys[(keys & np.uint32(0xFFFFFC00)) == np.uint32(prefix)] & np.uint32(0x3FF), minlength=1024), rank)
        return float(np.array([prefix | b2], np.uint32).view(F32)[0])

    bg = prev_bg = median()
    iterations_run, converged = 0, False
    for it in range(iterations):
        iterations_run = it + 1
        if abs(bg - target_background) < convergence_threshold:
            converged = True
            break
        if it > 0 and abs(bg - prev_bg) < convergence_threshold * 0.1:
            break
        m = F32(MR.mtf_balance(bg, target_background))
        st["pred_b0"] = int(np.ascontiguousarray(MR.apply_mtf(np.array([bg], F32), m)).view(np.uint32)[0]) >> 21
        st["pred_valid"] = bool(predict)
        blend = mask * protection
        working = (working * blend + MR.apply_mtf(working, m) * (F32(1.0) - blend)).astype(F32)
        keys = keys_of()
        st["pred_hist"] = np.bincount((keys[(keys >> np.uint32(21)) == st["pred_b0"]] >> np.uint32(10)) & np.uint32(0x7FF), minlength=2048)
        prev_bg, bg = bg, median()
    with np.errstate(invalid="ignore"):
        working = np.clip(working, F32(0.0), F32(1.0)).astype(F32)
    return working, iterations_run, bg, converged, trace
