"""numpy restatement of the colour finish: the three RGB packers (infra/render/rgb.rs:29-31, :71-77; core/compose/drizzle_rgb.rs:244-246),
process_drizzle_rgb (drizzle_rgb.rs:41-145) and the export command's stretch_and_render (cmd/export/mod.rs:357-409).

The packers are written out in np.float32 arithmetic.  The two pipelines are compositions of the oracle's existing functions
(compute_image_stats, select_wb_reference, auto_stf, compute_linked_stf, apply_stf_f32, apply_scnr, resample_image) with f32 numpy
for the crop, the multiply and the `/ 3.0` merge: no new C.  Pinned by tests/test_rgb_export_cpu.py; tests/test_gpu_rgb_export.py
holds the device to it, byte for byte and bit for bit.
"""
import numpy as np

F32 = np.float32
PACK_8, PACK_8_ROUND, PACK_16BE = 0, 1, 2
PACKS = (PACK_8, PACK_8_ROUND, PACK_16BE)

# the smallest shapes at which the kernel's cases differ: no group at all, a group with and without pixels around it, more than one
# row, more than one workgroup; BIG spans many workgroups with odd dims; TURN holds more four-pixel groups (563 569) than the largest
# grid has lanes (256 CUs x 8 workgroups x 256), so the grid-stride loop turns
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (2, 7), (5, 13), (16, 16), (33, 65)]
BIG = (257, 1031)
TURN = (1201, 1877)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the packers ---------------------------------------------------------------------------------------------------------------
def clamp01(v):
    """f32::clamp(0.0, 1.0): a NaN stays a NaN"""
    v = np.asarray(v, F32)
    return np.where(v < F32(0), F32(0), np.where(v > F32(1), F32(1), v)).astype(F32)


def round_half_away(x):
    """f32::round: the nearest integer, halves away from zero (np.round goes to even).  x - trunc(x) is exact in f32."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        return np.where(np.abs(x - t) >= F32(0.5), t + np.copysign(F32(1), x), t).astype(F32)


def as_unsigned(x, top):
    """Rust's `as u8` / `as u16` of an f32: truncates, saturates, NaN -> 0"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), F32(0), np.clip(x, F32(0), F32(top)))
        return np.trunc(y).astype(np.uint32)


def samples(v, pack):
    """one channel's samples as uint32"""
    with np.errstate(invalid="ignore"):
        if pack == PACK_16BE:
            return as_unsigned(clamp01(v) * F32(65535.0), 65535)
        x = clamp01(v) * F32(255.0)
        return as_unsigned(round_half_away(x) if pack == PACK_8_ROUND else x, 255)


def pack_rgb(r, g, b, pack):
    """interleaved R, G, B -> uint8 (rows, cols, 3); PACK_16BE: (rows, cols, 6), each sample high byte first"""
    q = np.stack([samples(c, pack) for c in (r, g, b)], axis=-1)
    if pack != PACK_16BE:
        return q.astype(np.uint8)
    out = np.empty(q.shape[:2] + (6,), np.uint8)
    out[..., 0::2] = q >> 8
    out[..., 1::2] = q & 255
    return out


# ---- process_drizzle_rgb (drizzle_rgb.rs:41-145) -------------------------------------------------------------------------------
def stats_tuple(st):
    return (st.min, st.max, st.median, st.mad, st.sigma, st.mean, st.valid_count)


def process_drizzle_rgb(oracle, r, g, b, white_balance="auto", auto_stretch=True, linked_stf=False, scnr=None):
    """-> dict(stretched, wb, rgb8, rows, cols, wb_factors, stf, chan_stats, stats_wb, scnr_applied); r / g / b: arrays or None"""
    present = [np.asarray(x, F32) for x in (r, g, b) if x is not None]
    rows = min(x.shape[0] for x in present)
    cols = min(x.shape[1] for x in present)
    img = [np.zeros((rows, cols), F32) if x is None else np.ascontiguousarray(np.asarray(x, F32)[:rows, :cols]) for x in (r, g, b)]  # :54-66
    full = [oracle.compute_image_stats(x) for x in img]  # :68-70
    if isinstance(white_balance, str):
        wb = oracle.select_wb_reference(*full) if white_balance == "auto" else (1.0, 1.0, 1.0)  # :76-80
    else:
        wb = tuple(float(v) for v in white_balance)
    with np.errstate(all="ignore"):
        wbp = [(x * F32(m)).astype(F32) for x, m in zip(img, wb)]  # :82-84
        if auto_stretch and linked_stf:  # :89-96
            combined = (((wbp[0] + wbp[1]) + wbp[2]) / F32(3.0)).astype(F32)
            p = oracle.auto_stf(oracle.compute_image_stats(combined))
            stf = [p, p, p]
            st = [oracle.compute_image_stats(x) for x in wbp]
        elif auto_stretch:  # :97-105
            st = [oracle.compute_image_stats(x) for x in wbp]
            stf = [oracle.auto_stf(s) for s in st]
        else:  # :106-116
            st = [oracle.compute_image_stats(x) for x in wbp]
            stf = [oracle.StfParams(0.0, 0.5, 1.0)] * 3
    s = [oracle.apply_stf_f32(x, p, q) for x, p, q in zip(wbp, stf, st)]  # :118-120
    if scnr is not None:  # :122-127
        s = list(oracle.apply_scnr(s[0], s[1], s[2], scnr.get("method", "average"), scnr.get("amount", 1.0), scnr.get("preserve_luminance", False)))
    return dict(stretched=s, wb=wbp, rgb8=pack_rgb(s[0], s[1], s[2], PACK_8_ROUND), rows=rows, cols=cols, wb_factors=tuple(wb),
                stf=[(p.shadow, p.midtone, p.highlight) for p in stf], chan_stats=[(f.min, f.max, f.median, f.mean) for f in full],
                stats_wb=[stats_tuple(q) for q in st], scnr_applied=scnr is not None)


# ---- stretch_and_render (cmd/export/mod.rs:357-409) ----------------------------------------------------------------------------
def stretch_and_render(oracle, r, g, b, bits_per_sample=16, stf=None):
    """-> (bytes, dict(rows, cols, resampled, stats, stf)); stf: three StfParams (the explicit branch) or None (linked)"""
    ch = [np.asarray(x, F32) for x in (r, g, b)]
    rows, cols = max(x.shape[0] for x in ch), max(x.shape[1] for x in ch)
    resampled = any(x.shape != (rows, cols) for x in ch)
    ch = [x if x.shape == (rows, cols) else oracle.resample_image(x, rows, cols) for x in ch]  # :396-407
    st = [oracle.compute_image_stats(x) for x in ch]  # :358-360
    if stf is None:
        linked, _ = oracle.compute_linked_stf(st[0], st[1], st[2])  # :371-378
        stf = [linked] * 3
    out = [oracle.apply_stf_f32(x, p, q) for x, p, q in zip(ch, stf, st)]
    data = pack_rgb(out[0], out[1], out[2], PACK_16BE if bits_per_sample == 16 else PACK_8)  # :381-382
    return data, dict(rows=rows, cols=cols, resampled=resampled, stats=[stats_tuple(q) for q in st],
                      stf=[(p.shadow, p.midtone, p.highlight) for p in stf])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def cases(shape):
    """name -> plane of `shape`, deterministic: what a packer and a stretch can meet"""
    rows, cols = shape
    n = rows * cols
    rng = np.random.default_rng(1000 * rows + cols)
    uniform = rng.random(n, dtype=F32)
    nasty = rng.random(n, dtype=F32)
    specials = [np.nan, np.inf, -np.inf, -0.25, 1.5, 2.0, 1e-7, 5e-8, 0.0, -0.0, 1.0, 1e-30]
    where = rng.permutation(n)[:max(1, min(n, max(len(specials), n // 7)))]
    nasty[where] = np.resize(np.array(specials, F32), where.size)
    ramp = ((np.arange(n, dtype=np.float64) % 255 + 0.5) / 255.0).astype(F32)   # round and truncate disagree at every sample
    out = {"uniform": uniform, "nasty": nasty, "constant": np.full(n, 0.375, F32), "ramp": ramp, "zero": np.zeros(n, F32)}
    return {k: np.ascontiguousarray(v.reshape(shape)) for k, v in out.items()}


TRIPLES = (("uniform", "nasty", "ramp"), ("constant", "zero", "uniform"), ("nasty", "ramp", "constant"))
