"""Plain Python restatement of the compose wizard's background step out of oracle.pyoracle: extract_background_cmd
(cmd/processing/background.rs:17-94) -- extract_background (:51), auto_stretch_preview of the corrected plane and of the model
(:53-54, cmd/common.rs:18-22), save_preview_png's nearest-neighbour pick of each (:65-66, cmd/common.rs:152-193) and the statistics the
command caches with the corrected plane (:73).  Python floats are IEEE doubles and Python's round() on x.5 differs from f64::round, so
round_half_away restates the latter.  Pinned by tests/test_background_step_cpu.py."""
import math
from dataclasses import dataclass

import numpy as np

MAX_PREVIEW_DIM = 4096          # cmd/common.rs:16


def round_half_away(x: float) -> float:
    """f64::round: half away from zero (x >= 0 here)"""
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else f


def pick_dims(width: int, height: int, max_dim: int):
    """downsample_nn's (dst_w, dst_h) (cmd/common.rs:158-164)"""
    if width <= max_dim and height <= max_dim:
        return width, height
    scale = float(max_dim) / float(max(width, height))
    dst_w = int(max(round_half_away(float(width) * scale), 1.0))
    dst_h = int(max(round_half_away(float(height) * scale), 1.0))
    return dst_w, dst_h


def pick_indices(n: int, dst: int):
    """the source index of every destination index along one axis: ((d as f64) * ratio).min((n - 1) as f64) as usize with
    ratio = n as f64 / dst as f64 (cmd/common.rs:166-176)"""
    ratio = float(n) / float(dst)
    return [int(min(float(d) * ratio, float(n - 1))) for d in range(dst)]


def downsample_nn(pixels: np.ndarray, max_dim: int) -> np.ndarray:
    """downsample_nn::<1> (cmd/common.rs:152-184) of a (height, width) byte plane"""
    height, width = pixels.shape
    dst_w, dst_h = pick_dims(width, height, max_dim)
    if (dst_w, dst_h) == (width, height):
        return pixels.copy()
    sy, sx = pick_indices(height, dst_h), pick_indices(width, dst_w)
    return np.ascontiguousarray(pixels[np.ix_(sy, sx)])     # out[dy, dx] = pixels[sy[dy], sx[dx]] (:171-181)


def auto_stretch_preview(oracle, plane):
    """auto_stretch_preview (cmd/common.rs:18-22) -> (bytes of every pixel, stats, stf)"""
    st = oracle.compute_image_stats(plane)
    stf = oracle.auto_stf(st)
    return oracle.apply_stf(plane, stf, st), st, stf


def preview_sampled(oracle, plane, max_dim=MAX_PREVIEW_DIM):
    """auto_stretch_preview followed by save_preview_png's pick -> (bytes, stats, stf)"""
    u8, st, stf = auto_stretch_preview(oracle, plane)
    return downsample_nn(u8, max_dim), st, stf


@dataclass
class Step:
    corrected: np.ndarray
    model: np.ndarray
    corrected_u8: np.ndarray
    model_u8: np.ndarray
    sample_count: int
    rms_residual: float
    coeffs: np.ndarray
    corrected_stats: object
    model_stats: object
    corrected_stf: object
    model_stf: object


def background_step(oracle, image, grid_size=8, poly_degree=3, sigma_clip=2.5, iterations=3, mode=0, max_dim=MAX_PREVIEW_DIM) -> Step:
    """extract_background_cmd's body (:51-73); raises ValueError with the reference's message like oracle.extract_background.  The
    statistics of :73 are compute_image_stats of the plane :53 already took them of: computed once here."""
    bg = oracle.extract_background(image, grid_size, poly_degree, sigma_clip, iterations, mode)
    cu8, cst, cstf = preview_sampled(oracle, bg.corrected, max_dim)
    mu8, mst, mstf = preview_sampled(oracle, bg.model, max_dim)
    return Step(bg.corrected, bg.model, cu8, mu8, bg.sample_count, bg.rms_residual, bg.coeffs, cst, mst, cstf, mstf)
