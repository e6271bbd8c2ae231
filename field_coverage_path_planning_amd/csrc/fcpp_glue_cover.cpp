// fcpp_glue_cover.cpp -- C-ABI glue of the coverage chain: polygon coverage, its regions, the patch passes over them (what the glue files do and share: fcpp_glue.h).
#include "fcpp_glue.h"
#include "fcpp_parallel.h"
#include "fcpp_patch.h"
#include "fcpp_patchfn.h"
#include "fcpp_pcover.h"
#include "fcpp_pcoverfn.h"
#include "fcpp_regionfn.h"
#include "fcpp_regions.h"

using namespace fcpp;

namespace {
// ---- polygon coverage (fcpp_pcover.hip; the rule: fcpp_pcoverfn.h) ----------------------------------------------------------------------
// what fcpp_polygon_cover_sizes, fcpp_polygon_cover and fcpp_debug_polygon_cover check alike
int pcover_args(int64_t n, const void *ring_offsets, int64_t n_rings, const void *vert_offsets, int64_t n_verts, const double *x, const double *y,
                double W, double res)
{
    if (!ring_offsets || !vert_offsets || (n_verts > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (const int bad = positive_finite(W, "width")) return bad;
    if (const int bad = positive_finite(res, "res")) return bad;
    if (n < 0 || n_rings < 0 || n_verts < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

int pcover_path_args(int64_t n, int caps, int64_t n_paths, const void *path_offsets, int64_t total_points, const double *x, const double *y,
                     const void *field_path_offsets)
{
    if (!path_offsets || !field_path_offsets || (total_points > 0 && (!x || !y))) return fail(FCPP_EINVAL, "bad arguments");
    if (caps != 0 && caps != 1) return fail(FCPP_EINVAL, "caps must be 0 (flat) or 1 (round)");
    if (n_paths < 0 || total_points < 0 || n_paths > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    return FCPP_OK;
}

// the fields' path offsets, read to the host and checked: start at 0, never decrease, name fewer than 2^31 paths
int pcover_field_paths(fcpp_ctx *c, int64_t n, const int64_t *ptr, std::vector<int64_t> &fpo)
{
    int rc = host_table(c, n + 1, ptr, (const int64_t *)nullptr, fpo);
    if (rc == FCPP_OK) rc = csr_ordered(fpo, n, "field_path_offsets");
    if (rc) return rc;
    if (fpo[(size_t)n] > ((int64_t)1 << 31)) return fail(FCPP_ESIZE, "field_path_offsets name 2^31 paths or more");
    return FCPP_OK;
}

// The paths of the fields, on the host and checked: poff (n_paths + 1), fpo (n + 1) and ids (fpo[n] entries, or NULL for the identity).
// -> the chunk table in field order and the fields' first chunks.
int pcover_chunks(int64_t n, int64_t n_paths, const std::vector<int64_t> &poff, const std::vector<int64_t> &fpo, const int64_t *ids,
                  std::vector<PcoverChunk> &chunks, std::vector<int64_t> &chunk_first)
{
    const int64_t S = fpo[(size_t)n];
    if (!ids && S > n_paths) return fail(FCPP_ESIZE, "field_path_offsets name more paths than there are");
    try {
        chunk_first.assign((size_t)n + 1, 0);
        chunks.clear();
        for (int64_t i = 0; i < n; ++i) {
            chunk_first[(size_t)i] = (int64_t)chunks.size();
            for (int64_t s = fpo[(size_t)i]; s < fpo[(size_t)i + 1]; ++s) {
                const int64_t p = ids ? ids[s] : s;
                if (p < 0 || p >= n_paths) return fail(FCPP_EINVAL, "path_ids must lie in [0, n_paths)");
                const int64_t p0 = poff[(size_t)p], p1 = poff[(size_t)p + 1];
                for (int64_t k = p0; k + 1 < p1; k += PCOVER_CHUNK)
                    chunks.push_back({ k, p0, p1, (int32_t)std::min<int64_t>(PCOVER_CHUNK, p1 - 1 - k), (int32_t)p });
            }
            if ((int64_t)chunks.size() > INT32_MAX) return fail(FCPP_ESIZE, "2^31 chunks of paths or more");
        }
        chunk_first[(size_t)n] = (int64_t)chunks.size();
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return FCPP_OK;
}

// ---- coverage regions (fcpp_regions.hip; the rule: fcpp_regionfn.h) ---------------------------------------------------------------------
// The grids of a call on the host, checked before any kernel runs: the fields' dims and cell offsets (the caller's host copy, or read
// back), and what the kernels place their work by: the fields' first tiles and first numbering blocks.
struct RegionTables {
    std::vector<RegionDims> dims;
    std::vector<int64_t> cells, tile_first, block_first;
};

int region_tables(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, RegionTables &T)
{
    if (n < 0 || n > INT32_MAX) return fail(FCPP_ESIZE, "bad sizes");
    try {
        T.dims.resize((size_t)n); T.cells.assign((size_t)n + 1, 0); T.tile_first.assign((size_t)n + 1, 0); T.block_first.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    int rc = host_copy_async(c, n, (const RegionDims *)dims, (const RegionDims *)nullptr, T.dims.data());
    if (rc == FCPP_OK) rc = host_copy_async(c, n + 1, cell_offsets, cell_offsets_host, T.cells.data());
    if (rc) return rc;
    if (c) HIPCHK(hipStreamSynchronize(c->stream));      // (one for both tables)
    if (T.cells[0] != 0) return fail(FCPP_ESIZE, "cell_offsets must start at 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t nx = T.dims[(size_t)i].nx, ny = T.dims[(size_t)i].ny, nc = T.cells[(size_t)i + 1] - T.cells[(size_t)i];
        if (nc < 0) return fail(FCPP_ESIZE, "cell_offsets must be non-decreasing");
        if (nx < 0 || ny < 0 || nx > REGION_MAX_CELLS || ny > REGION_MAX_CELLS || nx * ny > REGION_MAX_CELLS)
            return fail(FCPP_ESIZE, "a field's grid is negative or has more than 2^28 cells");
        if (nx * ny != nc) return fail(FCPP_ESIZE, "cell_offsets disagree with dims: a field's cells are not nx ny");
        T.tile_first[(size_t)i + 1] = T.tile_first[(size_t)i] + ((nx + REGION_TILE - 1) / REGION_TILE) * ((ny + REGION_TILE - 1) / REGION_TILE);
        T.block_first[(size_t)i + 1] = T.block_first[(size_t)i] + (nc + REGION_BLOCK_CELLS - 1) / REGION_BLOCK_CELLS;
    }
    if (T.tile_first[(size_t)n] > INT32_MAX || T.block_first[(size_t)n] > INT32_MAX) return fail(FCPP_ESIZE, "2^31 tiles or numbering blocks or more");
    return FCPP_OK;
}

// region offsets on the host, read and checked: start at 0, never decrease, end at n_regions
int region_csr(fcpp_ctx *c, int64_t n, const int64_t *ptr, const int64_t *host, int64_t n_regions, std::vector<int64_t> &ro)
{
    int rc = host_table(c, n + 1, ptr, host, ro);
    if (rc == FCPP_OK) rc = csr_ordered(ro, n, "region_offsets");
    if (rc) return rc;
    if (ro[(size_t)n] != n_regions) return fail(FCPP_ESIZE, "n_regions is not the total of region_offsets");
    return FCPP_OK;
}

struct RegionDevice {
    DevBuf<int64_t> tile_first, block_first, block_count, block_prefix, err;
    RegionFields F;
    int upload(fcpp_ctx *c, const RegionTables &T, const void *dims, const int64_t *cell_offsets)
    {
        HIPCHK(tile_first.upload(T.tile_first, c->stream));
        HIPCHK(block_first.upload(T.block_first, c->stream));
        HIPCHK(block_count.alloc((size_t)T.block_first.back()));
        HIPCHK(block_prefix.alloc((size_t)T.block_first.back() + 1));
        HIPCHK(err.alloc(1));
        F = { (const RegionDims *)dims, cell_offsets, tile_first.p, block_first.p };
        return FCPP_OK;
    }
};

// ---- patch passes (fcpp_patch.hip; the rule: fcpp_patchfn.h) ------------------------------------------------------------------------------
// what every patch entry checks of its scalars and its region offsets, before any kernel runs
int patch_call_args(fcpp_ctx *c, int64_t n, double res, double width, double margin, double join, const int64_t *offsets, const int64_t *offsets_host,
                    int64_t n_regions, std::vector<int64_t> &ro)
{
    if (!patch_args_ok(res, width, margin, join))
        return fail(FCPP_EINVAL, "res and width must be positive, 0 <= margin with width - 2 margin > 0, join >= 0, all finite");
    if (n < 0 || n > INT32_MAX || n_regions < 0) return fail(FCPP_ESIZE, "bad sizes");
    return region_csr(c, n, offsets, offsets_host, n_regions, ro);
}

// the field angles on the host, checked (patch_angle_ok is the swaths' range)
int patch_angles(fcpp_ctx *c, int64_t n, const double *angle, std::vector<double> &th)
{
    return host_angles(c, n, angle, nullptr, "a field's angle is not finite or beyond 1e5 in magnitude", th);
}

PatchRule patch_rule(double res, double width, double margin, double join) { return { res, width - 2.0 * margin, margin, patch_join_bins(join, res) }; }
}  // namespace

extern "C" {

int fcpp_polygon_cover_sizes(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                             const double *x, const double *y, double width, double res, void *dims, int64_t *cell_offsets,
                             int64_t *cell_offsets_host, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if (!dims || !cell_offsets) return fail(FCPP_EINVAL, "bad arguments");
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> rings, verts;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    return sample_counts(c, n, cell_offsets, cell_offsets_host, "the cells could not be scanned", [&](hipStream_t st, int64_t *err) {
        const int e = launch_pcover_sizes(st, n, ring_offsets, vert_offsets, x, y, width, res, (PcoverDims *)dims, status);
        return e ? e : launch_pcover_offsets(st, n, (const PcoverDims *)dims, cell_offsets, nullptr, err);
    });
}

// Like the path operators' fill entries, the cover call RECOMPUTES the grids from its inputs: the two entries stay stateless, and the
// kernels place every field by the offsets computed here -- the caller's offsets only have to end at the same total.
int fcpp_polygon_cover(fcpp_ctx *c, int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts,
                       const double *x, const double *y, double width, double res, int caps, int64_t n_paths, const int64_t *path_offsets,
                       const int64_t *path_offsets_host, int64_t total_points, const double *px, const double *py, const uint8_t *work,
                       const int32_t *pass, const int64_t *field_path_offsets, const int64_t *path_ids, const int64_t *cell_offsets,
                       const int64_t *cell_offsets_host, uint8_t *grid, int64_t *counts, int32_t *status)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !counts) || (grid && !cell_offsets && !cell_offsets_host)) return fail(FCPP_EINVAL, "bad arguments");
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc == FCPP_OK) rc = pcover_path_args(n, caps, n_paths, path_offsets, total_points, px, py, field_path_offsets);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<int64_t> rings, verts, poff, fpo, ids;
    rc = swath_fields(c, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc == FCPP_OK) rc = host_offsets(c, n_paths, path_offsets, path_offsets_host, total_points, "path_offsets", poff);
    if (rc == FCPP_OK) rc = pcover_field_paths(c, n, field_path_offsets, fpo);
    if (rc == FCPP_OK && path_ids) rc = host_table(c, fpo[(size_t)n], path_ids, (const int64_t *)nullptr, ids);      // (read only where there are any)
    if (rc) return rc;
    std::vector<PcoverChunk> chunks;
    std::vector<int64_t> chunk_first;
    rc = pcover_chunks(n, n_paths, poff, fpo, path_ids ? ids.data() : nullptr, chunks, chunk_first);
    if (rc) return rc;

    DevBuf<PcoverDims> dims;
    DevBuf<int64_t> cell_first, tile_first, err, d_chunk_first;
    DevBuf<int32_t> own_status;
    DevBuf<PcoverChunk> d_chunks;
    DevBuf<PcoverBox> boxes;
    HIPCHK(dims.alloc((size_t)n));
    HIPCHK(cell_first.alloc((size_t)n + 1));
    HIPCHK(tile_first.alloc((size_t)n + 1));
    HIPCHK(err.alloc(1));
    if (!status) { HIPCHK(own_status.alloc((size_t)n)); status = own_status.p; }
    LAUNCHCHK(launch_pcover_sizes(st, n, ring_offsets, vert_offsets, x, y, width, res, dims.p, status));
    LAUNCHCHK(launch_pcover_offsets(st, n, dims.p, cell_first.p, tile_first.p, err.p));
    int64_t totals[3] = { 0, 0, 0 };           // cells, tiles, the caller's cells
    HIPCHK(hipMemcpyAsync(&totals[0], cell_first.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&totals[1], tile_first.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (grid) {
        if (cell_offsets_host) totals[2] = cell_offsets_host[n];
        else HIPCHK(hipMemcpyAsync(&totals[2], cell_offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (n > 0) HIPCHK(hipMemsetAsync(counts, 0, (size_t)n * 4 * sizeof(int64_t), st));
    HIPCHK(d_chunks.upload(chunks, st));
    HIPCHK(d_chunk_first.upload(chunk_first, st));
    HIPCHK(boxes.alloc(chunks.size()));
    HIPCHK(hipStreamSynchronize(st));
    if (grid && totals[2] != totals[0]) return fail(FCPP_ESIZE, "cell_offsets do not end at the cells of these fields: call fcpp_polygon_cover_sizes");
    if (totals[1] > INT32_MAX) return fail(FCPP_ESIZE, "2^31 tiles or more");
    const PcoverPaths P = { px, py, work, pass };
    const PcoverFields F = { ring_offsets, vert_offsets, x, y, dims.p, cell_first.p, tile_first.p, d_chunk_first.p };
    LAUNCHCHK(launch_pcover_boxes(st, (int64_t)chunks.size(), d_chunks.p, P, boxes.p));
    LAUNCHCHK(launch_pcover_tiles(st, n, totals[1], F, width, res, caps, d_chunks.p, boxes.p, P, grid, (unsigned long long *)counts));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_debug_polygon_cover(int64_t n, const int64_t *ring_offsets, int64_t n_rings, const int64_t *vert_offsets, int64_t n_verts, const double *x,
                             const double *y, double width, double res, int caps, int64_t n_paths, const int64_t *path_offsets, int64_t total_points,
                             const double *px, const double *py, const uint8_t *work, const int32_t *pass, const int64_t *field_path_offsets,
                             const int64_t *path_ids, void *dims_out, int64_t *cell_offsets, int64_t cell_cap, uint8_t *grid, int64_t *counts,
                             int32_t *status)
{
    int rc = pcover_args(n, ring_offsets, n_rings, vert_offsets, n_verts, x, y, width, res);
    if (rc == FCPP_OK && counts) rc = pcover_path_args(n, caps, n_paths, path_offsets, total_points, px, py, field_path_offsets);
    if (rc == FCPP_OK && cell_cap < 0) rc = fail(FCPP_ESIZE, "bad sizes");
    if (rc) return rc;
    std::vector<int64_t> rings, verts, poff, fpo, cells;
    rc = swath_fields(nullptr, n, ring_offsets, nullptr, n_rings, vert_offsets, nullptr, n_verts, rings, verts);
    if (rc) return rc;
    std::vector<PcoverDims> dims;
    try { dims.resize((size_t)n); cells.assign((size_t)n + 1, 0); } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i) {
        const int st = pcover_field_dims_host(verts.data(), rings[(size_t)i], rings[(size_t)i + 1], x, y, width, res, dims[(size_t)i]);
        store(status, i, st);
        cells[(size_t)i + 1] = cells[(size_t)i] + dims[(size_t)i].nx * dims[(size_t)i].ny;
    }
    if (dims_out && n > 0) memcpy(dims_out, dims.data(), dims.size() * sizeof(PcoverDims));
    if (cell_offsets) memcpy(cell_offsets, cells.data(), cells.size() * sizeof(int64_t));
    if (!counts) return FCPP_OK;
    rc = host_offsets(nullptr, n_paths, path_offsets, nullptr, total_points, "path_offsets", poff);
    if (rc == FCPP_OK) rc = pcover_field_paths(nullptr, n, field_path_offsets, fpo);
    if (rc) return rc;
    std::vector<PcoverChunk> chunks;          // (built only for the checks the device entry makes: the same errors for the same arguments)
    std::vector<int64_t> chunk_first;
    rc = pcover_chunks(n, n_paths, poff, fpo, path_ids, chunks, chunk_first);
    if (rc) return rc;
    const bool want_grid = grid && cells[(size_t)n] <= cell_cap;
    const PcoverPaths P = { px, py, work, pass };
    // fields to the library's host threads: every field writes only its own counts and cells
    try {
        WorkerPool::parallel_for(n, [&](int64_t i) {
            const PcoverDims &d = dims[(size_t)i];
            const int64_t nc = d.nx * d.ny, r0 = rings[(size_t)i], r1 = rings[(size_t)i + 1];
            int64_t *cnt = counts + 4 * i;
            cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
            if (nc == 0) return;
            std::vector<uint8_t> own;
            std::vector<int32_t> first((size_t)nc);
            std::vector<double> cross((size_t)(verts[(size_t)r1] - verts[(size_t)r0]));
            uint8_t *bits = want_grid ? grid + cells[(size_t)i] : (own.resize((size_t)nc), own.data());
            pcover_field_host(verts.data(), r0, r1, x, y, d, width, res, caps, poff.data(), P, path_ids, fpo[(size_t)i], fpo[(size_t)i + 1], bits,
                              first.data(), cross.data(), cnt);
        });
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    return FCPP_OK;
}

int fcpp_cover_regions_counts(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host,
                              const uint8_t *grid, int mask, int value, int connectivity, int32_t *labels, int64_t *region_offsets,
                              int64_t *region_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !dims) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (!region_args_ok(mask, value, connectivity))
        return fail(FCPP_EINVAL, "mask and value must lie in 0 .. 255 with value & ~mask == 0, connectivity must be 4 or 8");
    HIPCHK(hipSetDevice(c->device));
    RegionTables T;
    int rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && (!grid || !labels)) return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    RegionDevice D;
    rc = D.upload(c, T, dims, cell_offsets);
    if (rc) return rc;
    const int64_t n_tiles = T.tile_first[(size_t)n], n_blocks = T.block_first[(size_t)n];
    LAUNCHCHK(launch_region_tiles(st, n, n_tiles, D.F, grid, mask, value, connectivity, labels));
    LAUNCHCHK(launch_region_seams(st, n, n_tiles, D.F, connectivity, labels, blocks_per_cu(c)));
    LAUNCHCHK(launch_region_count(st, n, n_blocks, D.F, 1, labels, D.block_count.p));
    LAUNCHCHK(launch_region_offsets(st, n, n_blocks, D.F, D.block_count.p, D.block_prefix.p, D.err.p, region_offsets));
    if (region_offsets_host)
        HIPCHK(hipMemcpyAsync(region_offsets_host, region_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

// Like the cover call, the fill call RECOMPUTES what it needs (the roots' ranks) from its inputs: nothing is kept in the context.
int fcpp_cover_regions_fill(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, int32_t *labels,
                            const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, void *records)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && !dims) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (n_regions < 0) return fail(FCPP_ESIZE, "bad sizes");
    HIPCHK(hipSetDevice(c->device));
    RegionTables T;
    int rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records)) return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    std::vector<int64_t> ro;
    rc = region_csr(c, n, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    RegionDevice D;
    rc = D.upload(c, T, dims, cell_offsets);
    if (rc) return rc;
    const int64_t n_blocks = T.block_first[(size_t)n];
    if (n_regions > 0) HIPCHK(hipMemsetAsync(records, 0, (size_t)n_regions * sizeof(RegionRecord), st));
    LAUNCHCHK(launch_region_count(st, n, n_blocks, D.F, 0, labels, D.block_count.p));
    LAUNCHCHK(launch_region_offsets(st, n, n_blocks, D.F, D.block_count.p, D.block_prefix.p, D.err.p, nullptr));
    LAUNCHCHK(launch_region_first(st, n, n_blocks, D.F, labels, D.block_prefix.p, region_offsets, (RegionRecord *)records));
    LAUNCHCHK(launch_region_fill(st, n, n_blocks, D.F, labels, region_offsets, (RegionRecord *)records));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_debug_cover_regions(int64_t n, const void *dims, const int64_t *cell_offsets, const uint8_t *grid, int mask, int value, int connectivity,
                             int64_t *region_offsets, int64_t region_cap, void *records, int32_t *labels_counts, int32_t *labels_fill)
{
    if ((n > 0 && !dims) || !cell_offsets) return fail(FCPP_EINVAL, "bad arguments");
    if (!region_args_ok(mask, value, connectivity))
        return fail(FCPP_EINVAL, "mask and value must lie in 0 .. 255 with value & ~mask == 0, connectivity must be 4 or 8");
    if (region_cap < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    const int rc = region_tables(nullptr, n, dims, cell_offsets, nullptr, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && !grid) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<std::vector<RegionRecord>> per;
    std::vector<int64_t> ro;
    // fields to the library's host threads: every field writes only its own records and labels
    try {
        per.resize((size_t)n); ro.assign((size_t)n + 1, 0);
        WorkerPool::parallel_for(n, [&](int64_t i) {
            const int64_t nx = T.dims[(size_t)i].nx, ny = T.dims[(size_t)i].ny, at = T.cells[(size_t)i];
            if (nx * ny == 0) return;
            std::vector<int32_t> parent((size_t)(nx * ny));
            region_field_host(grid + at, nx, ny, mask, value, connectivity, parent.data(), labels_counts ? labels_counts + at : nullptr,
                              labels_fill ? labels_fill + at : nullptr, per[(size_t)i]);
        });
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    for (int64_t i = 0; i < n; ++i) ro[(size_t)i + 1] = ro[(size_t)i] + (int64_t)per[(size_t)i].size();
    if (region_offsets) memcpy(region_offsets, ro.data(), ro.size() * sizeof(int64_t));
    if (records && ro[(size_t)n] <= region_cap)
        for (int64_t i = 0; i < n; ++i)
            if (!per[(size_t)i].empty())
                memcpy((RegionRecord *)records + ro[(size_t)i], per[(size_t)i].data(), per[(size_t)i].size() * sizeof(RegionRecord));
    return FCPP_OK;
}

int fcpp_patch_sizes(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, double res,
                     const int32_t *labels, const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, const double *angle,
                     double width, double margin, double join, double *frame, void *records, int64_t *totals_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !angle || !frame)) || !cell_offsets || !region_offsets || !totals_host) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    RegionTables T;
    rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records)) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<double> th;
    rc = patch_angles(c, n, angle, th);
    if (rc) return rc;
    hipStream_t st = c->stream;
    DevBuf<int64_t> block_first, line_first, word_first, err;
    HIPCHK(block_first.upload(T.block_first, st));
    HIPCHK(line_first.alloc((size_t)n_regions + 1));
    HIPCHK(word_first.alloc((size_t)n_regions + 1));
    HIPCHK(err.alloc(1));
    const PatchFields F = { (const RegionDims *)dims, cell_offsets, block_first.p, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    if (n_regions > 0) HIPCHK(hipMemsetAsync(records, 0, (size_t)n_regions * sizeof(PatchRecord), st));
    LAUNCHCHK(launch_patch_frame(st, n, angle, frame));
    if (n_regions > 0) LAUNCHCHK(launch_patch_extent(st, n, T.block_first[(size_t)n], F, rule, labels, (PatchRecord *)records));
    LAUNCHCHK(launch_patch_layout(st, n_regions, rule, (PatchRecord *)records, line_first.p, word_first.p, err.p));
    HIPCHK(hipMemcpyAsync(totals_host, line_first.p + n_regions, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(totals_host + 1, word_first.p + n_regions, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_patch_counts(fcpp_ctx *c, int64_t n, const void *dims, const int64_t *cell_offsets, const int64_t *cell_offsets_host, double res,
                      const int32_t *labels, const int64_t *region_offsets, const int64_t *region_offsets_host, int64_t n_regions, const double *frame,
                      double width, double margin, double join, const void *records, int64_t n_lines, int64_t n_words, uint64_t *bitmap,
                      int64_t *line_counts, int64_t *line_offsets, int64_t *swath_offsets, int64_t *swath_offsets_host)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !frame)) || !cell_offsets || !region_offsets || !line_offsets || !swath_offsets) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    if (n_lines < 0 || n_words < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    rc = region_tables(c, n, dims, cell_offsets, cell_offsets_host, T);
    if (rc) return rc;
    if ((T.cells[(size_t)n] > 0 && !labels) || (n_regions > 0 && !records) || (n_words > 0 && !bitmap) || (n_lines > 0 && !line_counts))
        return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    DevBuf<int64_t> block_first, err;
    HIPCHK(block_first.upload(T.block_first, st));
    HIPCHK(err.alloc(1));
    const PatchFields F = { (const RegionDims *)dims, cell_offsets, block_first.p, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    const PatchSwaths none = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    if (n_words > 0) HIPCHK(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint64_t), st));
    if (n_lines > 0) HIPCHK(hipMemsetAsync(line_counts, 0, (size_t)n_lines * sizeof(int64_t), st));
    if (n_regions > 0)
        LAUNCHCHK(launch_patch_mark(st, n, T.block_first[(size_t)n], F, rule, labels, (const PatchRecord *)records, n_words, (unsigned long long *)bitmap));
    LAUNCHCHK(launch_patch_runs(st, 0, n, n_regions, n_lines, n_words, F, rule, (const PatchRecord *)records, (const unsigned long long *)bitmap,
                                line_counts, nullptr, none, blocks_per_cu(c)));
    LAUNCHCHK(launch_patch_offsets(st, n, n_regions, n_lines, F, (const PatchRecord *)records, line_counts, line_offsets, err.p, swath_offsets));
    if (swath_offsets_host)
        HIPCHK(hipMemcpyAsync(swath_offsets_host, swath_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));          // (the tables die here)
    return FCPP_OK;
}

int fcpp_patch_fill(fcpp_ctx *c, int64_t n, const void *dims, double res, const int64_t *region_offsets, const int64_t *region_offsets_host,
                    int64_t n_regions, const double *frame, double width, double margin, double join, const void *records, int64_t n_lines,
                    int64_t n_words, const uint64_t *bitmap, const int64_t *line_offsets, int64_t n_swaths, double *ax, double *ay, double *bx, double *by,
                    int32_t *line, double *length, int64_t *region)
{
    if (!c) return fail(FCPP_EINVAL, "context is NULL");
    if ((n > 0 && (!dims || !frame)) || !region_offsets || !line_offsets) return fail(FCPP_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> ro;
    int rc = patch_call_args(c, n, res, width, margin, join, region_offsets, region_offsets_host, n_regions, ro);
    if (rc) return rc;
    if (n_lines < 0 || n_words < 0 || n_swaths < 0) return fail(FCPP_ESIZE, "bad sizes");
    if ((n_regions > 0 && !records) || (n_words > 0 && !bitmap) || (n_swaths > 0 && (!ax || !ay || !bx || !by || !line || !length || !region)))
        return fail(FCPP_EINVAL, "bad arguments");
    hipStream_t st = c->stream;
    int64_t total = 0;
    rc = table_ends(c, line_offsets, n_lines, nullptr, &total);
    if (rc) return rc;
    if (total != n_swaths) return fail(FCPP_ESIZE, "n_swaths is not the total of line_offsets");
    const PatchFields F = { (const RegionDims *)dims, nullptr, nullptr, region_offsets, frame };
    const PatchRule rule = patch_rule(res, width, margin, join);
    const PatchSwaths out = { ax, ay, bx, by, length, line, region, n_swaths };
    if (n_swaths > 0)
        LAUNCHCHK(launch_patch_runs(st, 1, n, n_regions, n_lines, n_words, F, rule, (const PatchRecord *)records, (const unsigned long long *)bitmap,
                                    nullptr, line_offsets, out, blocks_per_cu(c)));
    HIPCHK(hipStreamSynchronize(st));
    return FCPP_OK;
}

int fcpp_debug_patch_swaths(int64_t n, const void *dims, const int64_t *cell_offsets, double res, const int32_t *labels, const int64_t *region_offsets,
                            int64_t n_regions, const double *angle, double width, double margin, double join, double *frame, void *records,
                            int64_t *totals, int64_t word_cap, uint64_t *bitmap, int64_t line_cap, int64_t *line_counts, int64_t *line_offsets,
                            int64_t *swath_offsets, int64_t swath_cap, double *ax, double *ay, double *bx, double *by, int32_t *line, double *length,
                            int64_t *region)
{
    if ((n > 0 && (!dims || !angle)) || !cell_offsets || !region_offsets) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<int64_t> ro;
    int rc = patch_call_args(nullptr, n, res, width, margin, join, region_offsets, nullptr, n_regions, ro);
    if (rc) return rc;
    if (word_cap < 0 || line_cap < 0 || swath_cap < 0) return fail(FCPP_ESIZE, "bad sizes");
    RegionTables T;
    rc = region_tables(nullptr, n, dims, cell_offsets, nullptr, T);
    if (rc) return rc;
    if (T.cells[(size_t)n] > 0 && !labels) return fail(FCPP_EINVAL, "bad arguments");
    std::vector<double> th;
    rc = patch_angles(nullptr, n, angle, th);
    if (rc) return rc;
    PatchHost o;
    try {
        // fields to the library's host threads: every field writes only its own regions' keys, words, counts and swaths
        patch_host(n, T.dims.data(), T.cells.data(), res, labels, ro.data(), th.data(), width, margin, join,
                   [](int64_t cnt, auto fn) { WorkerPool::parallel_for(cnt, fn); }, o);
    } catch (const std::bad_alloc &) { return fail(FCPP_ENOMEM, "out of host memory"); }
    auto put = [](void *dst, const void *src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    put(frame, o.frame.data(), o.frame.size() * sizeof(double));
    put(records, o.records.data(), o.records.size() * sizeof(PatchRecord));
    if (totals) { totals[0] = o.n_lines; totals[1] = o.n_words; totals[2] = o.n_swaths; }
    put(swath_offsets, o.swath_offsets.data(), o.swath_offsets.size() * sizeof(int64_t));
    if (o.n_words <= word_cap) put(bitmap, o.bitmap.data(), o.bitmap.size() * sizeof(uint64_t));
    if (o.n_lines <= line_cap) {
        put(line_counts, o.line_counts.data(), o.line_counts.size() * sizeof(int64_t));
        put(line_offsets, o.line_offsets.data(), o.line_offsets.size() * sizeof(int64_t));
    }
    if (o.n_swaths <= swath_cap) {
        const size_t m8 = (size_t)o.n_swaths * sizeof(double);
        put(ax, o.ax.data(), m8); put(ay, o.ay.data(), m8); put(bx, o.bx.data(), m8); put(by, o.by.data(), m8); put(length, o.length.data(), m8);
        put(line, o.line.data(), (size_t)o.n_swaths * sizeof(int32_t));
        put(region, o.region.data(), (size_t)o.n_swaths * sizeof(int64_t));
    }
    return FCPP_OK;
}

}  // extern "C"
