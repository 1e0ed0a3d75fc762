// The device-to-device copy of one statistics chain's result out of the chain's state block (stats.hip: ab_stats_enqueue), before the
// next chain overwrites it.  Shared by the entry points that enqueue several chains back to back and read the results on the device:
// wizard_color.hip (the blend and colour steps) and compose_step.hip (the RGB Compose panel).  Launched with one small workgroup.
#pragma once
#include "ab_common.hpp"

namespace {

__global__ void save_stats_kernel(const ab_image_stats *st, ab_image_stats *dst) {
    if (threadIdx.x == 0) *dst = *st;
}

}  // namespace
