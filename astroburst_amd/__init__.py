"""astroburst_amd -- MI355X (gfx950) implementation of AstroBurst's pixel-compute hot path.

The product is astroburst_amd/libastroburst_hip.so (hand-written HIP behind the C ABI in
include/astroburst_hip.h).  `core` mirrors the reference's `core::*` Rust functions over that
ABI for tests and benchmarks; `synth` makes deterministic synthetic frame stacks.
"""
from ._lib import AstroBurstError, LIB_PATH, build, declared_symbols, is_dev_build, version  # noqa: F401
from .core import Comm, Context, ImageStats, PlaneList, PsfResult, PsfStar, StackResult, StfParams, psf_select_stars  # noqa: F401
from .core import ASINH_ROUTE_AVX2, ASINH_ROUTE_SCALAR, AsinhStats  # noqa: F401
from .core import RGB_PACK_8, RGB_PACK_8_ROUND, RGB_PACK_16BE, DrizzleRgbResult, ProcessedDrizzleRgb, RgbExportInfo, rgb_packed_bytes  # noqa: F401
from .core import ToneInfo, ToneResult  # noqa: F401
from .core import CROP_AUTO_THRESHOLD, CropBox, CropPlan  # noqa: F401
from .core import FitsView, RgbFitsView, downsample_histogram, histogram_bin_edges  # noqa: F401
from .core import COLOR_STATS_EXACT_OR_FULL, COLOR_STATS_KNOWN_RANGE, AutoWb, BlendCompositeResult, ColorPlan, ColorStepResult  # noqa: F401
from .core import color_step_plan, compute_auto_wb  # noqa: F401
from .core import MASK_PER_CHANNEL, MASK_SHARED_LUMINANCE, ArcsinhCompositeResult, ArcsinhViewResult, MaskedStretchCompositeResult  # noqa: F401
from .core import arcsinh_rgb_range  # noqa: F401
from .core import BackgroundStepResult  # noqa: F401
from .core import ComposeRgbResult  # noqa: F401
from .core import matches_from_votes, triangle_votes_host  # noqa: F401
from .core import SynthFrames, synth_chacha_block, synth_config, synth_noise_params, synth_psf_type, synth_rng_f64, synth_star_field  # noqa: F401
from .core import StackFrameParams, SubframeMetrics, stack_frame_params, stack_params_from_metrics  # noqa: F401

__version__ = "0.2.0"
