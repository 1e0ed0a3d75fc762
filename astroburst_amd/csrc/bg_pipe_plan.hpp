// The arithmetic of the background-tile pipeline (detect.hip: ab_bg_pipeline_*): the tile grid of a plane and the chunks a batch's planes
// are launched in.  Pure host arithmetic on <cstdint> / <cstddef> alone (tests/test_bg_pipe_plan_cpu.py builds it for the CPU and holds it
// to rows written out there).  Whoever needs a chunk's range or a plane's chunk -- the enqueue, the feeder thread, ab_bg_pipeline_get --
// asks PipeChunks: the formulas cannot drift apart.
#pragma once
#include <cstddef>
#include <cstdint>

// estimate_background's tiling (star_detection.rs:36-46): tiles of `step` px, row-major, the last row / column ragged
struct TileGrid {
    int64_t tile_size;
    int step, nty, ntx, ntiles;
};
// the grid of a caller's tile_size: step = max(tile_size, 16), ceiling divisions
inline TileGrid ab_tile_grid_of(int64_t rows, int64_t cols, int64_t tile_size) {
    TileGrid g;
    g.tile_size = tile_size;
    g.step = (int)(tile_size > 16 ? tile_size : 16);
    g.nty = (int)((rows + g.step - 1) / g.step);
    g.ntx = (int)((cols + g.step - 1) / g.step);
    g.ntiles = g.nty * g.ntx;
    return g;
}
// detect_stars' choice of tile_size (star_detection.rs:100): an eighth of the short side, 32 .. 256 px
inline TileGrid ab_tile_grid(int64_t rows, int64_t cols) {
    const int64_t eighth = (rows < cols ? rows : cols) / 8;
    return ab_tile_grid_of(rows, cols, eighth < 32 ? 32 : (eighth > 256 ? 256 : eighth));
}

// n planes in launches of `chunk`; the FIRST launch may be shorter (`first` planes: nothing else can run until the reference's and the
// first group's tiles are done).  first = 0: `chunk` like every launch.
struct PipeChunks {
    size_t n = 0, chunk = 1, first = 0, nchunks = 0;
    size_t begin(size_t c) const { return first ? (c == 0 ? 0 : first + (c - 1) * chunk) : c * chunk; }
    size_t count(size_t c) const {
        if (first && c == 0) return first;
        const size_t left = n - begin(c);
        return left < chunk ? left : chunk;
    }
    size_t chunk_of(size_t i) const { return first ? (i < first ? 0 : 1 + (i - first) / chunk) : i / chunk; }
};
// `first` counts only when 0 < first < chunk and first < n; a chunk below 1 is taken as 1 (the callers refuse it before they plan)
inline PipeChunks ab_pipe_chunks(size_t n, int chunk, int first) {
    PipeChunks p;
    p.n = n;
    p.chunk = chunk > 1 ? (size_t)chunk : 1;
    p.first = (first > 0 && first < chunk && (size_t)first < n) ? (size_t)first : 0;
    p.nchunks = p.first ? 1 + (n - p.first + p.chunk - 1) / p.chunk : (n + p.chunk - 1) / p.chunk;
    return p;
}
