// fcpp_slab.h -- a batch's device tables, described ONCE.  The tables live in one allocation (the "slab"; its host-built front part is the
// "image"); the list below names each with its element type and its element count, and everything else is derived from it: where each
// table begins (layout_image), typed pointers for a base address (bind_tables: the device slab, the host image BatchTiler::fill writes, the
// image a test reads back) and each table's byte length (slab_table).  A new table is one entry of the list, plus its users.
// Plain C++: the host tiler and the tests' sanitizer builds (g++, no HIP headers) include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_vector_types.h>
#endif

#include "fcpp_internal.h"

namespace fcpp {

// an element of field_junc: HIP's double2; without HIP a type of the same size and alignment (two doubles, 16 bytes) stands in for it
#ifdef __HIPCC__
typedef double2 FieldJunc;
#else
struct alignas(16) FieldJunc { double x, y; };
#endif

// X(name, element type, element count), counts in terms of the layout `L`.  The order within a part is the order in the slab.
// (chunks / span_chunks: k_plan_quiet's lists; red_paths has room for every field; red_scratch: 64 slice results of 104 bytes per field of
// class 3; partial: one slot per statistics entry; work_totals: per field of field_work the statistics of its quiet runs, summed once;
// info: the fcpp_field_info records of a batch set up on the device; own_stats: fcpp_batch_plan's statistics when the caller brings none)
#define FCPP_SLAB_HEAD(X)                                                                                                          \
    X(fields, DevField, L.n_fields) X(prims, DevPrim, L.n_prims) X(tiles, DevTile, L.n_tiles) X(wtiles, DevWaveTile, L.n_wave)     \
    X(general_ids, int32_t, L.n_general)
#define FCPP_SLAB_CHUNKS(X) X(chunks, DevTile, L.n_chunks) X(span_chunks, DevTile, L.n_span_chunks)
#define FCPP_SLAB_HOST(X)                                                                                                          \
    X(chunk_groups, DevChunkGroup, L.n_chunk_groups) X(stat_ids, int32_t, L.n_stat) X(stat_first, int64_t, L.n_fields + 1)         \
    X(stat_run, int64_t, L.n_stat) X(red_paths, int32_t, L.n_fields) X(field_work, DevFieldWork, L.n_field_work)                   \
    X(field_packs, DevFieldPack, L.n_field_work) X(open_wave_ids, int32_t, L.n_open_wave)                                          \
    X(obs_off, int64_t, L.n_polys > 0 ? L.n_polys + 1 : 0) X(obs_x, double, L.n_poly_verts) X(obs_y, double, L.n_poly_verts)       \
    X(obs_bbox, double, L.n_polys * 4) X(seg, double, L.n_fields * 8) X(seg_mask, int32_t, L.n_fields * 2)
#define FCPP_SLAB_DEVICE(X)                                                                                                        \
    X(partial, TilePartial, L.n_stat) X(red_scratch, char, L.n_red[3] * 64 * 104) X(field_junc, FieldJunc, L.n_fields)             \
    X(work_totals, TilePartial, L.n_field_work) X(info, fcpp_field_info, L.info_on_device ? L.n_fields : 0)                        \
    X(own_stats, fcpp_field_stats, L.n_fields)
#define FCPP_SLAB_TABLES(X) FCPP_SLAB_HEAD(X) FCPP_SLAB_CHUNKS(X) FCPP_SLAB_HOST(X) FCPP_SLAB_DEVICE(X)

// the counts of a batch's tables and, from them, where each table begins: offsets in bytes from the slab's start, 256-byte aligned
struct ImageLayout {
#define X(name, T, count) size_t name = 0;
    FCPP_SLAB_TABLES(X)
#undef X
    size_t upload_bytes = 0;                  // [0, upload_bytes) is built on the host and copied; behind it: device-only
    bool info_on_device = false;              // the batch was set up on the device: its fcpp_field_info records live in the slab (info)
    size_t total_bytes = 0;
    int64_t n_fields = 0, n_prims = 0, n_tiles = 0, n_wave = 0, n_general = 0, n_chunks = 0, n_span_chunks = 0, n_runs = 0, n_stat = 0;
    int64_t n_chunk_groups = 0;               // host-built images: the chunk lists are expanded on the device from this many groups (0: the lists are in the image)
    int64_t n_red[4] = { 0, 0, 0, 0 };       // fields reduced by k_reduce_stats, by class (fields of field_work are in none)
    int64_t n_field_work = 0, n_open_wave = 0;  // fields planned AND reduced by one workgroup each / wave tiles of the other fields
    int64_t n_polys = 0, n_poly_verts = 0;
    int64_t quiet_points = 0, span_points = 0, chunk_points = 0, wave_points = 0;
    int64_t work_wave_points = 0;             // the part of wave_points in fields of field_work
    int64_t unfusable_work = 0;               // fields of field work whose span has more than FUSED_SPAN_CHUNKS chunks
    int64_t work_span_points = 0;             // points of layer-1 spans written by k_plan_sparse_fields (not part of span_points: those are k_plan_quiet's)
    int64_t n_work[4] = { 0, 0, 0, 0 };       // fields of field_work by class (field_work_class: wavefronts of the workgroup); n_field_work = their sum
    int64_t wave_fail[5] = { 0, 0, 0, 0, 0 }; // diagnostics: stretches refused for wave tiles, by reason
    int64_t wave_inside = 0;                  // wave tiles whose outputs the host found inside the geofence
};

// The tables' places from their counts: the same for an image built on the host and one built on the device.  The chunk lists are part of
// the host-built image when the host wrote them (n_chunk_groups == 0) and lie behind it when the device expands them from the groups.
inline void layout_image(ImageLayout &L)
{
    size_t o = 0;
#define X(name, T, count) L.name = o; o = (o + (size_t)(count) * sizeof(T) + 255) & ~(size_t)255;
    FCPP_SLAB_HEAD(X)
    if (L.n_chunk_groups == 0) { FCPP_SLAB_CHUNKS(X) }
    FCPP_SLAB_HOST(X)
    L.upload_bytes = o;
    if (L.n_chunk_groups > 0) { FCPP_SLAB_CHUNKS(X) }
    FCPP_SLAB_DEVICE(X)
#undef X
    L.total_bytes = o;
}

// typed pointers to the tables ...
struct SlabTables {
#define X(name, T, count) T *name = nullptr;
    FCPP_SLAB_TABLES(X)
#undef X
};
// ... of the slab (or image) at `base`; a batch without obstacles has no obstacle tables
inline SlabTables bind_tables(const ImageLayout &L, void *base)
{
    SlabTables t;
    unsigned char *d = static_cast<unsigned char *>(base);
    if (!d) return t;
#define X(name, T, count) t.name = reinterpret_cast<T *>(d + L.name);
    FCPP_SLAB_TABLES(X)
#undef X
    if (L.n_polys <= 0) t.obs_off = nullptr, t.obs_x = t.obs_y = t.obs_bbox = nullptr;
    return t;
}

// one table by number (in the list's order): where it begins and its length in bytes
#define X(name, T, count) ST_##name,
enum SlabTable : int { FCPP_SLAB_TABLES(X) ST_COUNT };
#undef X
struct SlabSpan { size_t off, bytes; };
inline SlabSpan slab_table(const ImageLayout &L, SlabTable id)
{
    const SlabSpan spans[ST_COUNT] = {
#define X(name, T, count) { L.name, (size_t)(count) * sizeof(T) },
        FCPP_SLAB_TABLES(X)
#undef X
    };
    return spans[id];
}

}  // namespace fcpp
