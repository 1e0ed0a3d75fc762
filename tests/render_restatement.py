"""Plain numpy / Python restatement of the reference's preview, tile-pyramid and IPC renderers up to (not including) the PNG encoder,
written from the Rust and sharing nothing with oracle/ or csrc/:

    cmd/helpers.rs:204-322          render_rgb_preview, render_rgb_preview_with_stf
    infra/render/rgb.rs:7-34        render_rgb (the preview of a plane that fits max_dim)
    infra/render/tiles.rs:40-481    downsample_2x, render_tile, compute_num_levels, percentile_bounds, the two pyramids
    infra/ipc.rs:37-148             encode_with_header, encode_with_header_downsampled
    math/simd.rs:255-315            find_minmax_simd, both branches
    core/imaging/stf.rs:49-58,122-145   mtf, make_stf_u8_fn;  core/imaging/stats.rs:11-13  is_valid_pixel

Rust semantics that numpy does not have by default and that are therefore stated here once:
  * `f64::round` / `f32::round` round half AWAY from zero (np.round and Python's round go to even): rust_round, round_half_away;
  * `f64 as usize` and `f32 as u8` truncate, saturate and send NaN to 0: sat_usize, as_u8;
  * `f32::clamp` keeps a NaN (and a -0.0): clamp_f32.

Two decisions of the project are stated where they apply:
  * the SIGN of a zero data_min / data_max in the IPC header is unspecified (ipc_encode): the reference keeps the first zero of
    each 65536-pixel chunk (strict `<` / `>`, ipc.rs:47-48) and merges the chunks with f32::min / f32::max (:30-31), which fix no sign;
    compare those fields by value;
  * percentile_bounds' fallback is find_minmax_simd's PORTABLE branch (simd.rs:263-271, is_finite); its AVX2 branch (:276-315) tests
    `v == v` on the whole chunks of eight and so keeps infinities.  Both are stated; test_render_restatement_cpu.py names a plane on
    which they differ.
"""
import math
import struct

import numpy as np

F32 = np.float32
F64 = np.float64
F32_MAX = F32(np.finfo(np.float32).max)
CUT = F32(1e-7)                      # types/constants.rs:6 PADDING_THRESHOLD, and tiles.rs:153's literal: both f32
IPC_CHUNK = 65536                    # ipc.rs:42


# ---- the three conversions --------------------------------------------------------------------------------------------------------
def rust_round(v: float) -> float:
    """f64::round: half away from zero (v - trunc(v) is exact, so no `+ 0.5` rounding trap)"""
    if not math.isfinite(v):
        return v
    t = float(math.trunc(v))
    return t + math.copysign(1.0, v) if abs(v - t) >= 0.5 else t


def sat_usize(v: float) -> int:
    """`f64 as usize`: truncating, saturating, NaN -> 0"""
    if not v > 0.0:
        return 0
    if v >= 18446744073709551616.0:
        return (1 << 64) - 1
    return int(v)


def round_half_away(x):
    """f32::round of an array, half away from zero; carried in f64, where x - trunc(x) is exact; +-inf and NaN pass through"""
    x64 = np.asarray(x, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x64)
        out = np.where(np.abs(x64 - t) >= 0.5, t + np.copysign(1.0, x64), t)
    return out.astype(F32)


def clamp_f32(v, lo, hi):
    """f32::clamp: `if v < lo { lo } else if v > hi { hi } else { v }` -- a NaN (and a -0.0 at lo = 0) stays"""
    v = np.asarray(v, F32)
    out = v.copy()
    with np.errstate(invalid="ignore"):
        out[v < F32(lo)] = F32(lo)
        out[v > F32(hi)] = F32(hi)
    return out


def as_u8(x):
    """`f32 as u8` / `f64 as u8`: truncating, saturating, NaN -> 0"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), 0.0, np.minimum(np.maximum(x, 0.0), 255.0))
    return np.trunc(y).astype(np.uint8)


# ---- make_stf_u8_fn (stf.rs:122-145) ----------------------------------------------------------------------------------------------
def make_stf_u8(params, stats):
    """params: (shadow, midtone, highlight) or an object with those fields; stats: an object with .min / .max (f64) -> f(array) -> u8"""
    shadow, midtone, highlight = params if isinstance(params, tuple) else (params.shadow, params.midtone, params.highlight)
    inv_range = 1.0 / max(float(stats.max) - float(stats.min), 1e-30)              # :123-126
    dmin = float(stats.min)
    inv_clip = 1.0 / max(float(highlight) - float(shadow), 1e-15)                  # :129-132
    m = float(midtone)

    def fn(v):
        v = np.asarray(v, F32)
        with np.errstate(all="ignore"):
            valid = np.isfinite(v) & (v > CUT)                                     # stats.rs:11-13
            vd = v.astype(F64)
            norm = (vd - dmin) * inv_range
            t = (norm - shadow) * inv_clip
            clipped = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))            # f64::clamp
            mid = (m - 1.0) * clipped / ((2.0 * m - 1.0) * clipped - m)            # mtf, :50-58
            stretched = np.where(clipped <= 0.0, 0.0, np.where(clipped >= 1.0, 1.0, mid))
            s = stretched * 255.0
            tr = np.trunc(s)
            r = np.where(np.abs(s - tr) >= 0.5, tr + np.copysign(1.0, s), tr)      # f64::round
            return np.where(valid, as_u8(r), 0).astype(np.uint8)
    return fn


# ---- previews (helpers.rs:204-322, rgb.rs:7-34) -----------------------------------------------------------------------------------
def preview_dims(rows: int, cols: int, max_dim: int):
    """-> (ph, pw, y_ratio, x_ratio); helpers.rs:216,224-229 == :282-289 == ipc.rs:107,112-117"""
    if rows <= max_dim and cols <= max_dim:
        return rows, cols, 1.0, 1.0
    scale = float(max_dim) / float(max(rows, cols))
    pw = sat_usize(max(rust_round(float(cols) * scale), 1.0))
    ph = sat_usize(max(rust_round(float(rows) * scale), 1.0))
    return ph, pw, float(rows) / float(ph), float(cols) / float(pw)


def nn_products(n_out: int, ratio: float):
    """(d as f64) * ratio for d in 0..n_out"""
    return np.arange(n_out, dtype=F64) * F64(ratio)


def nn_index(n_out: int, ratio: float, length: int):
    """((d as f64) * ratio).min((len - 1) as f64) as usize  (helpers.rs:237,240)"""
    return np.minimum(nn_products(n_out, ratio), F64(length - 1)).astype(np.int64)


def lands_on_integers(rows, cols, max_dim) -> bool:
    """whether some d * ratio with d > 0 is an exact integer in a SCALED preview (where a ratio one ulp off would pick another pixel)"""
    ph, pw, yr, xr = preview_dims(rows, cols, max_dim)
    if rows <= max_dim and cols <= max_dim:
        return False
    py, px = nn_products(ph, yr)[1:], nn_products(pw, xr)[1:]
    return bool((py == np.floor(py)).any() or (px == np.floor(px)).any())


def u8_truncated(v):
    """(v.clamp(0.0, 1.0) * 255.0) as u8  (helpers.rs:243, rgb.rs:29)"""
    with np.errstate(invalid="ignore"):
        return as_u8(clamp_f32(v, 0.0, 1.0) * F32(255.0))


def u8_rounded(v):
    """(v.clamp(0.0, 1.0) * 255.0).round() as u8  (tiles.rs:291)"""
    with np.errstate(invalid="ignore"):
        return as_u8(round_half_away(clamp_f32(v, 0.0, 1.0) * F32(255.0)))


def render_rgb_preview(r, g, b, max_dim: int, stf=None, stats=None):
    """-> (ph, pw, 3) u8; stf / stats: three each for render_rgb_preview_with_stf, None for the plain map"""
    rows, cols = r.shape
    ph, pw, yr, xr = preview_dims(rows, cols, max_dim)
    sy, sx = nn_index(ph, yr, rows), nn_index(pw, xr, cols)
    out = np.zeros((ph, pw, 3), np.uint8)
    for c, ch in enumerate((r, g, b)):
        picked = np.asarray(ch, F32)[np.ix_(sy, sx)]
        out[:, :, c] = u8_truncated(picked) if stf is None else make_stf_u8(stf[c], stats[c])(picked)
    return out


# ---- IPC buffer (ipc.rs:37-148) ---------------------------------------------------------------------------------------------------
def _first_min_max(values):
    """strict `<` / `>` from (f32::MAX, f32::MIN): the FIRST occurrence of the extreme value (this is what fixes a zero's sign)"""
    if values.size == 0:
        return F32_MAX, -F32_MAX
    mn, mx = values[np.argmin(values)], values[np.argmax(values)]
    return (mn if mn < F32_MAX else F32_MAX), (mx if mx > -F32_MAX else -F32_MAX)


def ipc_encode(arr, max_dim: int = 0) -> bytes:
    """encode_with_header (max_dim == 0, or the plane fits: ipc.rs:107-109) / encode_with_header_downsampled.  The sign of a zero
    data_min / data_max is UNSPECIFIED (module docstring); what is returned here is the first-met zero within a chunk and the earlier
    chunk's on a tie between chunks."""
    a = np.asarray(arr, F32)
    rows, cols = a.shape
    if max_dim == 0 or (rows <= max_dim and cols <= max_dim):
        flat = a.ravel()
        mn, mx = F32_MAX, -F32_MAX
        for s in range(0, flat.size, IPC_CHUNK):                                   # :41-55
            chunk = flat[s:s + IPC_CHUNK]
            cmn, cmx = _first_min_max(chunk[np.isfinite(chunk)])
            mn, mx = (cmn if cmn < mn else mn), (cmx if cmx > mx else mx)
        clean = np.where(np.isfinite(flat), flat, F32(0.0)).astype("<f4")          # :63-73 (the raw copy is the same bytes)
        ph, pw = rows, cols
    else:
        ph, pw, yr, xr = preview_dims(rows, cols, max_dim)                         # :112-117
        picked = a[np.ix_(nn_index(ph, yr, rows), nn_index(pw, xr, cols))].ravel()
        clean = np.where(np.isfinite(picked), picked, F32(0.0)).astype("<f4")      # :130
        mn, mx = _first_min_max(clean)                                             # :131-132: over the CLEANED samples
    dmin, dmax = (F32(0.0), F32(1.0)) if mn > mx else (mn, mx)                     # :57-58, :137-138
    return struct.pack("<II", pw, ph) + np.array([dmin, dmax], "<f4").tobytes() + clean.tobytes()


# ---- tiles (tiles.rs) -------------------------------------------------------------------------------------------------------------
def _cells(a):
    rows, cols = a.shape
    nr, nc = (rows + 1) // 2, (cols + 1) // 2
    y0, x0 = np.arange(nr) * 2, np.arange(nc) * 2
    y1, x1 = np.minimum(y0 + 1, rows - 1), np.minimum(x0 + 1, cols - 1)            # :50,53: the last row / column counts twice
    return [a[np.ix_(y0, x0)], a[np.ix_(y0, x1)], a[np.ix_(y1, x0)], a[np.ix_(y1, x1)]]   # a, b, c, d  (:54-57)


def downsample_2x(data):
    """tiles.rs:40-70: the f64 sum goes strictly in a, b, c, d order over the finite members"""
    q = _cells(np.asarray(data, F32))
    s = np.zeros(q[0].shape, F64)
    cnt = np.zeros(q[0].shape, np.int64)
    for m in q:                                                                    # :60-63
        fin = np.isfinite(m)
        s = np.where(fin, s + np.where(fin, m, F32(0.0)).astype(F64), s)
        cnt += fin
    with np.errstate(all="ignore"):
        return np.where(cnt > 0, (s / np.maximum(cnt, 1).astype(F64)).astype(F32), F32(0.0)).astype(F32)   # :64


def downsample_2x_pairwise(data):
    """NOT the reference: (a + b) + (c + d).  Only there to show that a fixture tells the two orders apart."""
    q = [np.where(np.isfinite(m), m, F32(0.0)).astype(F64) for m in _cells(np.asarray(data, F32))]
    cnt = sum(np.isfinite(m).astype(np.int64) for m in _cells(np.asarray(data, F32)))
    with np.errstate(all="ignore"):
        return np.where(cnt > 0, (((q[0] + q[1]) + (q[2] + q[3])) / np.maximum(cnt, 1).astype(F64)).astype(F32), F32(0.0)).astype(F32)


def find_minmax_portable(flat):
    """simd.rs:263-271"""
    flat = np.asarray(flat, F32).ravel()
    fin = flat[np.isfinite(flat)]
    return (F32_MAX, -F32_MAX) if fin.size == 0 else (min(F32_MAX, fin.min()), max(-F32_MAX, fin.max()))


def find_minmax_avx2(flat):
    """simd.rs:276-315: `v == v` (keeps +-inf) on the whole chunks of eight, is_finite on the remainder"""
    flat = np.asarray(flat, F32).ravel()
    whole = (flat.size // 8) * 8
    head, tail = flat[:whole], flat[whole:]
    keep = np.concatenate([head[head == head], tail[np.isfinite(tail)]])
    return (F32_MAX, -F32_MAX) if keep.size == 0 else (min(F32_MAX, keep.min()), max(-F32_MAX, keep.max()))


def valid_pixels(flat):
    """tiles.rs:150-154: v.is_finite() && *v > 1e-7, the literal an f32"""
    flat = np.asarray(flat, F32).ravel()
    with np.errstate(invalid="ignore"):
        return flat[np.isfinite(flat) & (flat > CUT)]


def percentile_ranks(n: int, low_pct: float, high_pct: float):
    """tiles.rs:162-163: ((n as f64 * pct) as usize).min(n - 1) -> (lo_idx, hi_idx)"""
    return min(sat_usize(float(n) * float(low_pct)), n - 1), min(sat_usize(float(n) * float(high_pct)), n - 1)


def percentile_bounds(data, low_pct: float = 0.001, high_pct: float = 0.999, fallback=find_minmax_portable):
    """tiles.rs:149-178 -> (lo, hi) as f32"""
    valid = valid_pixels(data)
    if valid.size == 0:                                                            # :156-159
        lo, hi = fallback(data)
        return F32(lo), F32(hi)
    lo_idx, hi_idx = percentile_ranks(valid.size, low_pct, high_pct)
    s = np.sort(valid)
    return s[lo_idx], s[hi_idx]


def compute_num_levels(width: int, height: int, tile_size: int) -> int:
    """tiles.rs:137-147"""
    max_dim, ts = float(max(width, height)), float(tile_size)
    if max_dim <= ts:
        return 1
    return max(sat_usize(math.ceil(math.log2(max_dim / ts))) + 1, 1)


def pyramid_layout(rows: int, cols: int, ts: int, channels: int):
    """tiles.rs:194-246 -> (levels, total bytes): level 0 is the coarsest; packed in level order, tiles in (ty, tx) order, every tile
    ts x ts x channels bytes -- the library's packing (ab_tile_pyramid_layout), computed here on its own"""
    nl = compute_num_levels(cols, rows, ts)
    dims = [(rows, cols)]
    for _ in range(1, nl):                                                         # :199-202 with downsample_2x's dims (:42-43)
        r, c = dims[-1]
        dims.append(((r + 1) // 2, (c + 1) // 2))
    levels, total = [], 0
    for level in range(nl):
        k = nl - 1 - level                                                         # stack_idx = max_level - level (:207)
        r, c = dims[k]
        tc, tr = (c + ts - 1) // ts, (r + ts - 1) // ts                            # :211-212
        levels.append(dict(level=level, width=c, height=r, cols=tc, rows=tr, scale_factor=1.0 / float(1 << k), offset=total))
        total += tc * tr * ts * ts * channels
    return levels, total


def pyramid_padded_tiles(rows, cols, ts, channels=1) -> int:
    """tiles, over all levels, whose ts x ts buffer is not wholly inside its level's image"""
    levels, _ = pyramid_layout(rows, cols, ts, channels)
    n = 0
    for L in levels:
        full_c, full_r = L["width"] // ts, L["height"] // ts
        n += L["cols"] * L["rows"] - full_c * full_r
    return n


def mono_bytes(level, gmin, gmax):
    """render_tile's pixel map (tiles.rs:96-110) over a whole level"""
    v = np.asarray(level, F32)
    gmin, gmax = F32(gmin), F32(gmax)
    with np.errstate(all="ignore"):
        d = F32(gmax - gmin)
        rng = d if d > F32(1e-10) else F32(1e-10)                                   # f32::max: a NaN difference gives 1e-10
        inv_range = F32(255.0) / rng
        t = round_half_away((v - gmin) * inv_range)
        return np.where(np.isfinite(v), as_u8(clamp_f32(t, 0.0, 255.0)), 0).astype(np.uint8)


def tile_buffers(level_bytes, ts: int):
    """every tile buffer of a level, zero outside the image, in (ty, tx) order: (rows, cols[, 3]) u8 -> flat bytes"""
    h, w = level_bytes.shape[:2]
    ch = level_bytes.shape[2:]
    tr, tc = (h + ts - 1) // ts, (w + ts - 1) // ts
    pad = np.zeros((tr * ts, tc * ts) + ch, np.uint8)                              # vec![0u8; ...]  (:99, :283)
    pad[:h, :w] = level_bytes
    pad = pad.reshape((tr, ts, tc, ts) + ch)
    return np.ascontiguousarray(np.swapaxes(pad, 1, 2)).ravel()


def render_tile(level, tx, ty, ts, gmin, gmax):
    """one render_tile buffer (tiles.rs:72-113) -> (ts, ts) u8"""
    h, w = level.shape
    buf = np.zeros((ts, ts), np.uint8)
    y0, x0 = ty * ts, tx * ts
    y1, x1 = min(y0 + ts, h), min(x0 + ts, w)
    if y1 > y0 and x1 > x0:
        buf[:y1 - y0, :x1 - x0] = mono_bytes(level[y0:y1, x0:x1], gmin, gmax)
    return buf


def generate_tile_pyramid(normalized, ts: int):
    """tiles.rs:179-255 up to the encoder -> (packed u8, levels, (gmin, gmax))"""
    a = np.asarray(normalized, F32)
    gmin, gmax = percentile_bounds(a, 0.001, 0.999)                                # :189
    levels, total = pyramid_layout(a.shape[0], a.shape[1], ts, 1)
    out = np.zeros(total, np.uint8)
    cur = a
    for L in reversed(levels):                                                     # finest first, as the stack is built (:196-202)
        assert cur.shape == (L["height"], L["width"])
        buf = tile_buffers(mono_bytes(cur, gmin, gmax), ts)
        out[L["offset"]:L["offset"] + buf.size] = buf
        if L["level"] > 0:
            cur = downsample_2x(cur)
    return out, levels, (float(gmin), float(gmax))


def generate_tile_pyramid_rgb(r, g, b, ts: int, stf=None, stats=None):
    """tiles.rs:363-481 up to the encoder (render_tile_rgb :257-298, render_tile_rgb_stf :300-341) -> (packed u8, levels)"""
    cur = [np.asarray(x, F32) for x in (r, g, b)]
    levels, total = pyramid_layout(cur[0].shape[0], cur[0].shape[1], ts, 3)
    fns = [u8_rounded] * 3 if stf is None else [make_stf_u8(stf[c], stats[c]) for c in range(3)]
    out = np.zeros(total, np.uint8)
    for L in reversed(levels):
        assert cur[0].shape == (L["height"], L["width"])
        buf = tile_buffers(np.stack([fns[c](cur[c]) for c in range(3)], axis=-1), ts)
        out[L["offset"]:L["offset"] + buf.size] = buf
        if L["level"] > 0:
            cur = [downsample_2x(x) for x in cur]                                  # :412-426
    return out, levels
