"""numpy restatement of the bicubic sampler and its three callers, written from the Rust and importing nothing from oracle/:

  catmull_rom, bicubic_sample   core/imaging/sampling.rs:4-14, 48-80
  clamp_index                   core/imaging/boundary.rs:9-20
  shift_image_subpixel          core/stacking/align.rs:36-57
  warp_image (+ map)            core/alignment/affine.rs:74-80, 663-690
  resample_image                core/imaging/resample.rs:25-61

f64 throughout, only the final store is f32.  The reference's operation order is kept (`row_val += s * w` per tap starting from 0.0,
`val += row_val * wy` starting from 0.0); catmull_rom takes the reference's own branch on |t| (a NaN falls through both compares to
0.0), not the statically split form of resample.hip; the in-bounds tests are the reference's f64 compares, not compares of integer
floors.  numpy evaluates one operation per pass and never fuses, so every intermediate is a correctly rounded f64 like the Rust's.

Everything works in row chunks of about CHUNK_PIXELS output pixels: a 13 759 x 12 451 warp needs the source, the output and a few
hundred MB of temporaries.

`f64 as i64` saturates and maps NaN to 0 (to_i64).  The reference then forms `ix + i - 1` in i64, which would overflow for a saturated
index; no caller reaches the sampler with such a coordinate except a NaN shift (index 0), so the index is limited to +-2^62 first,
which changes no clamped tap."""
import numpy as np

CHUNK_PIXELS = 1 << 21
_IGNORE = dict(over="ignore", invalid="ignore", under="ignore")


def catmull_rom(t):
    """sampling.rs:4-14 on an array (or a scalar)"""
    with np.errstate(**_IGNORE):
        abs_t = np.abs(np.asarray(t, np.float64))
        inner = abs_t * abs_t * (1.5 * abs_t - 2.5) + 1.0
        outer = abs_t * (abs_t * (2.5 - 0.5 * abs_t) - 4.0) + 2.0
        return np.where(abs_t <= 1.0, inner, np.where(abs_t <= 2.0, outer, 0.0))


def to_i64(v):
    """Rust's `f64 as i64`: saturating, NaN -> 0"""
    v = np.asarray(v, np.float64)
    out = np.zeros(v.shape, np.int64)
    hi, lo = v >= 9223372036854775807.0, v <= -9223372036854775808.0
    mid = ~(hi | lo | np.isnan(v))
    out[mid] = v[mid].astype(np.int64)
    out[hi] = np.iinfo(np.int64).max
    out[lo] = np.iinfo(np.int64).min
    return out


def clamp_index(idx, length):
    """boundary.rs:9-20 on an int64 array"""
    if length == 0:
        return np.zeros_like(idx)
    return np.where(idx < 0, 0, np.where(idx >= length, length - 1, idx))


def bicubic_sample(src, y, x):
    """sampling.rs:48-80 at the coordinates y, x (f64 arrays that broadcast against each other) -> f32 array"""
    src = np.asarray(src, np.float32)
    rows, cols = src.shape
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    shape = np.broadcast(y, x).shape
    if rows == 0 or cols == 0:
        return np.zeros(shape, np.float32)
    with np.errstate(**_IGNORE):
        ix, iy = to_i64(np.floor(x)), to_i64(np.floor(y))
        fx, fy = x - ix.astype(np.float64), y - iy.astype(np.float64)
        ix, iy = np.clip(ix, -(1 << 62), 1 << 62), np.clip(iy, -(1 << 62), 1 << 62)
        wx = [catmull_rom(fx + 1.0), catmull_rom(fx), catmull_rom(fx - 1.0), catmull_rom(fx - 2.0)]
        val = np.zeros(shape, np.float64)
        for j in range(4):
            r = clamp_index(iy + (j - 1), rows)
            row_val = np.zeros(shape, np.float64)
            for i in range(4):
                c = clamp_index(ix + (i - 1), cols)
                row_val = row_val + src[r, c].astype(np.float64) * wx[i]
            val = val + row_val * catmull_rom(fy - float(j - 1))
        return val.astype(np.float32)


def _chunks(n_rows, n_cols):
    step = max(1, CHUNK_PIXELS // max(n_cols, 1))
    for r0 in range(0, n_rows, step):
        yield r0, min(r0 + step, n_rows)


def shift_coords(rows, cols, dy, dx):
    """align.rs:46-51 -> (sy per row, sx per column, rows that sample, columns that sample)"""
    sy = np.arange(rows, dtype=np.float64) + float(dy)
    sx = np.arange(cols, dtype=np.float64) + float(dx)
    with np.errstate(**_IGNORE):
        ok_y = ~((sy < -0.5) | (sy > float(rows) - 0.5))
        ok_x = ~((sx < -0.5) | (sx > float(cols) - 0.5))
    return sy, sx, ok_y, ok_x


def shift_image_subpixel(image, dy, dx):
    """align.rs:36-57"""
    image = np.asarray(image, np.float32)
    if abs(float(dy)) < 1e-12 and abs(float(dx)) < 1e-12:
        return image.copy()
    rows, cols = image.shape
    sy, sx, ok_y, ok_x = shift_coords(rows, cols, dy, dx)
    out = np.zeros((rows, cols), np.float32)
    xs = np.nonzero(ok_x)[0]
    if xs.size == 0:
        return out
    for r0, r1 in _chunks(rows, cols):
        ys = r0 + np.nonzero(ok_y[r0:r1])[0]
        if ys.size:
            out[np.ix_(ys, xs)] = bicubic_sample(image, sy[ys][:, None], sx[xs][None, :])
    return out


def warp_coords(transform, src_rows, src_cols, out_cols, row0, row1):
    """affine.rs:74-80 and the test of :675-679 for output rows [row0, row1) -> (sx, sy, inside), each (row1 - row0, out_cols)"""
    a, b, tx, c, d, ty = (float(v) for v in transform)
    x = np.arange(out_cols, dtype=np.float64)[None, :]
    y = np.arange(row0, row1, dtype=np.float64)[:, None]
    with np.errstate(**_IGNORE):
        sx = a * x + b * y + tx
        sy = c * x + d * y + ty
        inside = (sx >= 0.0) & (sy >= 0.0) & (sx < float(src_cols - 1)) & (sy < float(src_rows - 1))
    return sx, sy, inside


def warp_image(image, transform, out_rows, out_cols, row0=0, nrows=None):
    """affine.rs:663-690; rows [row0, row0 + nrows) of it when a band is asked for"""
    image = np.asarray(image, np.float32)
    src_rows, src_cols = image.shape
    nrows = out_rows - row0 if nrows is None else nrows
    out = np.zeros((nrows, out_cols), np.float32)
    for r0, r1 in _chunks(nrows, out_cols):
        sx, sy, inside = warp_coords(transform, src_rows, src_cols, out_cols, row0 + r0, row0 + r1)
        if inside.any():
            out[r0:r1][inside] = bicubic_sample(image, sy[inside], sx[inside])
    return out


def resample_coords(src_rows, src_cols, target_rows, target_cols):
    """resample.rs:41-44, 52, 54 -> (sy per target row, sx per target column)"""
    scale_y = float(src_rows) / float(target_rows)
    scale_x = float(src_cols) / float(target_cols)
    half_shift_y = (scale_y - 1.0) * 0.5
    half_shift_x = (scale_x - 1.0) * 0.5
    sy = np.arange(target_rows, dtype=np.float64) * scale_y + half_shift_y
    sx = np.arange(target_cols, dtype=np.float64) * scale_x + half_shift_x
    return sy, sx


def resample_image(image, target_rows, target_cols):
    """resample.rs:25-61"""
    image = np.asarray(image, np.float32)
    src_rows, src_cols = image.shape
    if target_rows == 0 or target_cols == 0:
        raise ValueError("Target dimensions must be > 0")
    if (target_rows, target_cols) == (src_rows, src_cols):
        return image.copy()
    sy, sx = resample_coords(src_rows, src_cols, target_rows, target_cols)
    out = np.empty((target_rows, target_cols), np.float32)
    for r0, r1 in _chunks(target_rows, target_cols):
        out[r0:r1] = bicubic_sample(image, sy[r0:r1, None], sx[None, :])
    return out


# ---- which of the sampler's classes a set of coordinates populates (for tests that must not silently test nothing) -----------------
def sampler_classes(sx, sy, sampled, rows, cols, wave=64):
    """Counts over the pixels of an output plane.  sx, sy broadcast to the plane's shape, `sampled` says which pixels reach
    bicubic_sample.  A wave is `wave` consecutive output columns of one row (pieces of 256 or 512 columns start on multiples of it):
    resample.hip takes the unclamped footprint when every sampled lane of a wave is interior, the clamped one otherwise."""
    sx, sy, sampled = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64), np.asarray(sampled, bool))
    with np.errstate(**_IGNORE):
        fx, fy = np.floor(sx), np.floor(sy)
        ix, iy = to_i64(fx), to_i64(fy)
        frx, fry = sx - fx, sy - fy
    interior = (ix >= 1) & (ix + 2 < cols) & (iy >= 1) & (iy + 2 < rows)
    s = sampled
    h, w = s.shape
    pad = (-w) % wave
    grp = lambda m, fill: np.pad(m, ((0, 0), (0, pad)), constant_values=fill).reshape(h, -1, wave)
    live = grp(np.ones((h, w), bool), False)
    g_s, g_int = grp(s, False), grp(interior, False)
    fast = (g_int | ~g_s | ~live).all(axis=2)
    any_s = g_s.any(axis=2)
    return dict(
        sampled=int(s.sum()), outside=int((~s).sum()), interior=int((s & interior).sum()), edge=int((s & ~interior).sum()),
        frac_zero_x=int((s & (frx == 0.0)).sum()), frac_zero_y=int((s & (fry == 0.0)).sum()),
        ix_first=int((s & (ix == 0)).sum()), ix_last=int((s & (ix == cols - 2)).sum()), ix_beyond=int((s & (ix >= cols - 1)).sum()),
        ix_negative=int((s & (ix < 0)).sum()),
        iy_first=int((s & (iy == 0)).sum()), iy_last=int((s & (iy == rows - 2)).sum()), iy_beyond=int((s & (iy >= rows - 1)).sum()),
        iy_negative=int((s & (iy < 0)).sum()),
        waves_unclamped=int((fast & any_s).sum()), waves_clamped=int((~fast).sum()),
        waves_clamped_mixed=int((~fast & (g_s & g_int).any(axis=2)).sum()),
        waves_partly_outside=int((any_s & (~g_s & live).any(axis=2)).sum()),
    )
