"""The background pipeline's arithmetic (astroburst_amd/csrc/bg_pipe_plan.hpp) against rows written out here, on the host alone.

ab_tile_grid() is the tile grid of estimate_background for detect_stars' choice of tile size; ab_pipe_chunks() cuts a batch's planes into
the launches of the tile pipeline and answers which launch holds a plane.  The enqueue, the feeder thread and ab_bg_pipeline_get all ask
the same struct, so one wrong formula would make a worker wait for the wrong launch's event: this test compiles a few lines around the
header with the host compiler and compares with rows that were worked out by hand from the launch code as it was before the header
existed (min(max(min(rows, cols) / 8, 32), 256), step = max(tile, 16), ceiling divisions; chunk c of a short first launch begins at
first + (c - 1) * chunk), not by calling the functions under test.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")

HARNESS = r"""
#include "bg_pipe_plan.hpp"
#include <cstdio>
#include <cstring>
int main() {
    char what[8];
    while (scanf("%7s", what) == 1) {
        if (!strcmp(what, "grid")) {
            long long rows, cols;
            if (scanf("%lld %lld", &rows, &cols) != 2) return 1;
            const TileGrid g = ab_tile_grid(rows, cols);
            const TileGrid h = ab_tile_grid_of(rows, cols, g.tile_size);  // the second half alone, on the first half's tile size
            printf("%lld %d %d %d %d %d %d %d %d\n", (long long)g.tile_size, g.step, g.nty, g.ntx, g.ntiles, h.step, h.nty, h.ntx, h.ntiles);
        } else {
            unsigned long n; int chunk, first;
            if (scanf("%lu %d %d", &n, &chunk, &first) != 3) return 1;
            const PipeChunks p = ab_pipe_chunks(n, chunk, first);
            printf("%lu %lu", (unsigned long)p.first, (unsigned long)p.nchunks);
            for (size_t c = 0; c < p.nchunks; ++c) printf(" %lu %lu", (unsigned long)p.begin(c), (unsigned long)p.count(c));
            printf(" |");
            for (size_t i = 0; i < n; ++i) printf(" %lu", (unsigned long)p.chunk_of(i));
            printf("\n");
        }
    }
    return 0;
}
"""

# (rows, cols) -> (step, nty, ntx, ntiles)
GRIDS = {
    (4096, 4096): (256, 16, 16, 256),
    (2048, 2048): (256, 8, 8, 64),
    (2047, 3000): (255, 9, 12, 108),
    (300, 403): (37, 9, 11, 99),
    (100, 5000): (32, 4, 157, 628),
    (3, 3): (32, 1, 1, 1),
}
# (n, chunk, first) -> (effective first, [(begin, end) ...])
CHUNKS = {
    (64, 16, 5): (5, [(0, 5), (5, 21), (21, 37), (37, 53), (53, 64)]),
    (5, 16, 5): (0, [(0, 5)]),
    (6, 16, 5): (5, [(0, 5), (5, 6)]),
    (22, 16, 5): (5, [(0, 5), (5, 21), (21, 22)]),
    (8, 8, 5): (5, [(0, 5), (5, 8)]),
    (64, 4, 0): (0, [(4 * c, 4 * c + 4) for c in range(16)]),
    (7, 4, 0): (0, [(0, 4), (4, 7)]),
    (9, 16, 0): (0, [(0, 9)]),
    (9, 16, 16): (0, [(0, 9)]),
}
CHUNK_OF = {(64, 16, 5): {4: 0, 5: 1, 20: 1, 21: 2, 63: 4}}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("bg_pipe_plan")
    src = os.path.join(tmp, "plan_harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(tmp, "plan_harness")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)

    def ask(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
        return [line for line in out.split("\n") if line]
    return ask


def test_the_header_needs_nothing_but_the_standard_integer_types():
    includes = [line.split()[1] for line in open(os.path.join(CSRC, "bg_pipe_plan.hpp")) if line.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>"], includes


def test_tile_grids(harness):
    got = harness([f"grid {r} {c}" for r, c in GRIDS])
    assert len(got) == len(GRIDS)
    for (dims, want), line in zip(GRIDS.items(), got):
        v = tuple(int(x) for x in line.split())
        assert v[1:5] == want, (dims, v, want)
        assert v[0] == want[0], (dims, v)  # the tile size: never below 32, so it is the step
        assert v[5:9] == want, ("from the tile size alone", dims, v, want)


def parse(line):
    head, tail = line.split("|")
    h = [int(x) for x in head.split()]
    first, nchunks, flat = h[0], h[1], h[2:]
    ranges = [(flat[2 * c], flat[2 * c] + flat[2 * c + 1]) for c in range(nchunks)]
    return first, ranges, [int(x) for x in tail.split()]


def test_chunks(harness):
    got = harness([f"chunks {n} {chunk} {first}" for n, chunk, first in CHUNKS])
    assert len(got) == len(CHUNKS)
    for (case, (want_first, want_ranges)), line in zip(CHUNKS.items(), got):
        first, ranges, chunk_of = parse(line)
        assert first == want_first, (case, first)
        assert ranges == want_ranges, (case, ranges)
        for i, c in CHUNK_OF.get(case, {}).items():
            assert chunk_of[i] == c, (case, i, chunk_of[i], c)


def test_every_plane_lies_in_its_chunk_and_the_counts_sum_to_n(harness):
    got = harness([f"chunks {n} {chunk} {first}" for n, chunk, first in CHUNKS])
    for (n, _, _), line in zip(CHUNKS, got):
        _, ranges, chunk_of = parse(line)
        assert sum(e - b for b, e in ranges) == n, (n, ranges)
        assert len(chunk_of) == n
        for i, c in enumerate(chunk_of):
            assert 0 <= c < len(ranges) and ranges[c][0] <= i < ranges[c][1], (n, i, c, ranges)
