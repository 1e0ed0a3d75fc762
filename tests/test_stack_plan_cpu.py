"""The stack planner (astroburst_amd/csrc/stack_plan.hpp) against the route table, on the host alone.

ab_stack_plan() is the one place that decides which of the six stacking engines a stack of n frames takes, and it is plain C++ over
<cstdint>: this test compiles a few lines around it with the host compiler and compares every field of the plan with rows WRITTEN OUT
below.  The rows come from the route table in the header (read off the launch code as it was before the planner existed), not from
calling the planner.  A planned route that changes -- a frame-count class, a list kernel, the single- / two-pass decision -- fails
here without a GPU; tests/test_gpu_stack.py then holds the kernels the plan names to the oracle.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")

HARNESS = r"""
#include "stack_plan.hpp"
#include <cstdio>
#include <cstring>
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "grid")) {  // lanes total -> the fast pass's wave count and pixels per wave
        int lanes; long long total;
        while (scanf("%d %lld", &lanes, &total) == 2) {
            const StackLanesGrid g = ab_stack_lanes_grid(lanes, total);
            printf("%lld %lld\n", (long long)g.waves, (long long)g.px_wave);
        }
        return 0;
    }
    unsigned long n; long long total; int contiguous, partial, median, exact, deep_from, aligned16;
    while (scanf("%lu %lld %d %d %d %d %d %d", &n, &total, &contiguous, &partial, &median, &exact, &deep_from, &aligned16) == 8) {
        const StackPlan p = ab_stack_plan(n, total, contiguous, partial, median, exact, deep_from, aligned16);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", p.engine, p.lanes, p.np, p.h, p.k, p.r, (int)p.pad_inf, (int)p.direct, (int)p.two_pass, p.list,
               p.gather, (int)p.tree);
    }
    return 0;
}
"""
# the enumerators of stack_plan.hpp, in order
SINGLE, LANE, PAIR, LANES, WIDE, DEEP = range(6)
NO_LIST, GENERAL, PAIR128, PAIR256, WIDE16 = range(5)
SCALAR, QUAD4, TILED = range(3)
FIELDS = ("engine", "lanes", "np", "h", "k", "r", "pad_inf", "direct", "two_pass", "list", "gather", "tree")


def row(engine, lanes=0, np=0, h=0, k=0, r=0, pad_inf=0, direct=0, two_pass=0, list=NO_LIST, gather=SCALAR, tree=0):
    return (engine, lanes, np, h, k, r, int(pad_inf), int(direct), int(two_pass), list, gather, int(tree))


def single():
    return row(SINGLE, lanes=1)


def lane(np, pad=False, direct=True, two=False):
    """one lane per pixel, NP samples: +inf pads up to NP, the DIRECT gather, fast pass + general pass"""
    return row(LANE, lanes=1, np=np, pad_inf=pad, direct=direct, two_pass=two, list=GENERAL if two else NO_LIST)


def duo(r):
    return row(LANES, lanes=2, h=128, r=r, pad_inf=1, two_pass=1, list=PAIR128)


def quad(lanes, r):
    return row(LANES, lanes=lanes, h=256, r=r, pad_inf=1, two_pass=1, list=PAIR256 if lanes == 4 else WIDE16)


def pair(h):
    return row(PAIR, lanes=2, h=h, r=h, pad_inf=1)


def wide(k, gather, tree):
    return row(WIDE, lanes=64, k=k, gather=gather, tree=tree)


def deep():
    return row(DEEP)


COUNTS = (1, 2, 3, 7, 8, 37, 64, 65, 100, 128, 129, 160, 161, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
TOTAL = 64 * 64  # contiguous, 16-byte aligned planes of 4096 pixels: whole groups of 4 .. 32 pixels for the 16-byte gathers

# setting -> (contiguous, partial, median, exact), {n: expected plan}; stack_deep_from = 4096
DEFAULT = {
    1: single(), 2: lane(2), 3: lane(4, direct=False), 7: lane(8, pad=True), 8: lane(8, two=True), 37: lane(64, pad=True), 64: lane(64, two=True),
    65: lane(128, pad=True), 100: lane(128, pad=True), 128: lane(128, two=True),
    129: duo(80), 160: duo(80), 161: duo(96), 256: duo(128),
    257: quad(4, 80), 512: quad(4, 128), 513: quad(8, 80), 1024: quad(8, 128),
    1025: wide(32, TILED, True), 2048: wide(32, TILED, True), 2049: wide(64, TILED, True), 4096: wide(64, TILED, True), 4097: deep(),
}
EXACT = {
    1: single(), 2: lane(2), 3: lane(4, direct=False), 7: lane(8, pad=True), 8: lane(8), 37: lane(64, pad=True), 64: lane(64),
    65: wide(2, QUAD4, False), 100: wide(2, QUAD4, False), 128: wide(2, QUAD4, False),
    129: pair(128), 160: pair(128), 161: pair(128), 256: pair(128), 257: pair(256), 512: pair(256),
    513: wide(16, TILED, False), 1024: wide(16, TILED, False), 1025: wide(32, TILED, False), 2048: wide(32, TILED, False),
    2049: wide(64, TILED, False), 4096: wide(64, TILED, False), 4097: deep(),
}
MEDIAN = {
    1: single(), 2: lane(2), 3: lane(4, direct=False), 7: lane(8, pad=True), 8: lane(8), 37: lane(64, pad=True), 64: lane(64),
    65: lane(128, pad=True), 100: lane(128, pad=True), 128: lane(128),
    129: duo(80), 160: duo(80), 161: duo(96), 256: duo(128),
    257: quad(4, 80), 512: quad(4, 128), 513: quad(8, 80), 1024: quad(8, 128),
    1025: wide(32, TILED, True), 2048: wide(32, TILED, True), 2049: wide(64, TILED, True), 4096: wide(64, TILED, True), 4097: deep(),
}
PARTIAL = {  # (sum, count) planes of the frame-sharded stack, contiguous frames
    1: single(), 2: lane(2), 3: lane(4, direct=False), 7: lane(8, pad=True), 8: lane(8, two=True), 37: lane(64, pad=True), 64: lane(64, two=True),
    65: wide(2, QUAD4, False), 100: wide(2, QUAD4, False), 128: wide(2, QUAD4, False),
    129: wide(4, QUAD4, False), 160: wide(4, QUAD4, False), 161: wide(4, QUAD4, False), 256: wide(4, QUAD4, False),
    257: wide(8, TILED, False), 512: wide(8, TILED, False), 513: wide(16, TILED, False), 1024: wide(16, TILED, False),
    1025: wide(32, TILED, False), 2048: wide(32, TILED, False), 2049: wide(64, TILED, False), 4096: wide(64, TILED, False), 4097: deep(),
}
RAGGED = {  # some row stride differs from the output's columns (a top-left crop), full output, default engine
    1: single(), 2: lane(2, direct=False), 3: lane(4, direct=False), 7: lane(8, direct=False), 8: lane(8, direct=False), 37: lane(64, direct=False),
    64: lane(64, direct=False),
    65: wide(2, SCALAR, True), 100: wide(2, SCALAR, True), 128: wide(2, SCALAR, True),
    129: wide(4, SCALAR, True), 160: wide(4, SCALAR, True), 161: wide(4, SCALAR, True), 256: wide(4, SCALAR, True),
    257: wide(8, SCALAR, True), 512: wide(8, SCALAR, True), 513: wide(16, SCALAR, True), 1024: wide(16, SCALAR, True),
    1025: wide(32, SCALAR, True), 2048: wide(32, SCALAR, True), 2049: wide(64, SCALAR, True), 4096: wide(64, SCALAR, True), 4097: deep(),
}
SETTINGS = {
    "default": ((1, 0, 0, 0), DEFAULT),
    "exact": ((1, 0, 0, 1), EXACT),
    "median": ((1, 0, 1, 0), MEDIAN),
    "partial": ((1, 1, 0, 0), PARTIAL),
    "ragged": ((0, 0, 0, 0), RAGGED),
}
# (n, total, contiguous, partial, median, exact, deep_from, aligned16) -> plan: the lowered threshold of the deep engine (the tests'
# AB_STACK_DEEP_FROM=64) and the alignment facts of the wave-per-pixel gathers
EXTRA = [
    # everything deeper than one lane's registers goes to the workgroup-per-pixel engine; the NP = 128 lane route keeps 65 .. 128
    # plain frames, as it always has
    ((64, TOTAL, 1, 0, 0, 0, 64, 1), lane(64, two=True)),
    ((65, TOTAL, 1, 0, 0, 0, 64, 1), lane(128, pad=True)),
    ((128, TOTAL, 1, 0, 0, 0, 64, 1), lane(128, two=True)),
    ((129, TOTAL, 1, 0, 0, 0, 64, 1), deep()),
    ((512, TOTAL, 1, 0, 1, 0, 64, 1), deep()),
    ((65, TOTAL, 1, 0, 0, 1, 64, 1), deep()),
    ((65, TOTAL, 1, 1, 0, 0, 64, 1), deep()),
    ((65, TOTAL, 0, 0, 0, 0, 64, 1), deep()),
    ((64, TOTAL, 0, 0, 0, 0, 64, 1), lane(64, direct=False)),
    # 16-byte loads need aligned planes and whole quads; the LDS-staged form whole groups of 256 / K pixels
    ((100, TOTAL, 1, 1, 0, 0, 4096, 0), wide(2, SCALAR, False)),
    ((100, TOTAL + 2, 1, 1, 0, 0, 4096, 1), wide(2, SCALAR, False)),
    ((300, TOTAL + 4, 1, 1, 0, 0, 4096, 1), wide(8, QUAD4, False)),   # 4100 pixels: quads, but no groups of 32
    ((600, TOTAL + 4, 1, 1, 0, 0, 4096, 1), wide(16, SCALAR, False)),  # no groups of 16, and no four-pixel form beyond 512 frames
    ((3000, TOTAL + 4, 0, 0, 0, 0, 4096, 1), wide(64, SCALAR, True)),
    ((3000, TOTAL + 4, 1, 0, 0, 0, 4096, 1), wide(64, TILED, True)),  # groups of 4
    # 2^30 pixels and more: byte offsets no longer fit 32 bits -- no DIRECT gather, no pads, no multi-lane engines
    ((64, 1 << 30, 1, 0, 0, 0, 4096, 1), lane(64, direct=False)),
    ((37, 1 << 30, 1, 0, 0, 0, 4096, 1), lane(64, direct=False)),
    ((100, 1 << 30, 1, 0, 0, 0, 4096, 1), wide(2, QUAD4, True)),
    ((200, 1 << 30, 1, 0, 0, 0, 4096, 1), wide(4, QUAD4, True)),
]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("stack_plan")
    src = os.path.join(tmp, "plan_harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(tmp, "plan_harness")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)

    def plan(cases, *mode):
        text = "".join(" ".join(str(int(x)) for x in c) + "\n" for c in cases)
        out = subprocess.run([exe, *mode], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        return [tuple(int(x) for x in line.split()) for line in out if line]
    return plan


def explain(got, want):
    return {f: (g, w) for f, g, w in zip(FIELDS, got, want) if g != w}


def test_the_header_needs_nothing_but_the_standard_integer_types():
    includes = [line.split()[1] for line in open(os.path.join(CSRC, "stack_plan.hpp")) if line.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>"], includes


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_routes_at_every_boundary(planner, setting):
    (contiguous, partial, median, exact), rows = SETTINGS[setting]
    assert tuple(sorted(rows)) == COUNTS
    got = planner([(n, TOTAL, contiguous, partial, median, exact, 4096, 1) for n in COUNTS])
    assert len(got) == len(COUNTS)
    wrong = {n: explain(g, rows[n]) for n, g in zip(COUNTS, got) if g != rows[n]}
    assert not wrong, f"{setting}: field -> (planned, expected): {wrong}"


def test_frame_count_classes(planner):
    """the spot values of R: frames per lane rounded up to a multiple of 16"""
    want = {129: 80, 160: 80, 161: 96, 256: 128, 257: 80, 512: 128, 513: 80, 1024: 128}
    got = planner([(n, TOTAL, 1, 0, 0, 0, 4096, 1) for n in want])
    assert {n: g[FIELDS.index("r")] for n, g in zip(want, got)} == want


def test_lowered_deep_threshold_alignment_and_large_planes(planner):
    got = planner([c for c, _ in EXTRA])
    wrong = {c: explain(g, w) for (c, w), g in zip(EXTRA, got) if g != w}
    assert len(got) == len(EXTRA) and not wrong, f"field -> (planned, expected): {wrong}"


# (lanes, total) -> (waves, pixels per wave) of the multi-lane fast pass: one wave per 64 / lanes pixels, the wave count rounded up to a
# multiple of 8 (the kernel deals neighbouring pixel groups to the workgroup ids of one XCD).  Written out, not computed.
LANES_GRID = {
    (2, 1): (8, 32), (2, 31): (8, 32), (2, 32): (8, 32), (2, 33): (8, 32), (2, 4100): (136, 32), (2, 1 << 24): (524288, 32),
    (4, 1): (8, 16), (4, 31): (8, 16), (4, 32): (8, 16), (4, 33): (8, 16), (4, 4100): (264, 16), (4, 1 << 24): (1048576, 16),
    (8, 1): (8, 8), (8, 31): (8, 8), (8, 32): (8, 8), (8, 33): (8, 8), (8, 4100): (520, 8), (8, 1 << 24): (2097152, 8),
}


def test_the_fast_pass_grid(planner):
    """ab_stack_lanes_grid: the one place the launch takes its grid from and the list set-up its capacity"""
    got = planner(list(LANES_GRID), "grid")
    assert dict(zip(LANES_GRID, got)) == LANES_GRID
