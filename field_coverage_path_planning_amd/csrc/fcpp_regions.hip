// fcpp_regions.hip -- gfx950 (MI355X) kernels of the coverage regions (include/fcpp.h: fcpp_cover_regions_counts, fcpp_cover_regions_fill):
// connected-component labelling of a batch of byte grids.  The rule is fcpp_regionfn.h; every value is an integer and the result is a function
// of the input alone, so the kernels give what fcpp_debug_cover_regions gives on the host, whatever the order the hardware works in.
// Plain C++: no inline assembly, integer atomics only (add, min, max), no spin waits, every loop bounded.
//
// THE FOREST.  labels[c] is cell c's PARENT, a field-local index, -1 for a non-member.  Two invariants hold from the first store to the last:
// a parent is never above its cell, and a root is its own parent.  So a find from c ends within c steps, the root of a set is its smallest
// cell -- the region's key -- and a word another workgroup reads while it is written is always an ancestor that was valid at some time
// (every such access is a relaxed atomic load, store or min: no torn or cached-stale word, nobody waits for anybody).
//
// k_region_tiles   a workgroup of 256 per 64 x 64 tile, fcpp_pcover.hip's layout (thread t: column t & 63, rows (t >> 6) + 4 q).  A row's
//                  membership is ONE ballot; every member starts at the first cell of its horizontal run (from the ballot's bits: no
//                  atomics), so only the vertical links remain: the first cell of every overlap of two rows' runs unions with N (under
//                  connectivity 8 also NW / NE where N is no member) by atomicMin in LDS.  Then every member reads up to its root and stores
//                  the root's field-local index.  LDS 16.5 KiB: 4096 parents, 64 row words.
// k_region_seams   lanes over the first column and the first row of every tile (128 per tile): each unions its cell with the members
//                  across the seam (W or N; under 8 also the two diagonals across it) in global memory.  A launch of at most `max_blocks`
//                  workgroups strides over the seam lanes.
// k_region_count   a workgroup per numbering block (4096 consecutive cells of ONE field, a wavefront per 1024): with `flatten` every member
//                  reads up to its root and stores it; the block's roots (labels[c] == c) are counted.  The samplers' scan
//                  (fcpp_samplefn.h, as it is) turns the counts into prefixes, k_region_offsets reads them at the fields' first blocks.
// k_region_first   the same blocks: the k-th root of a field, in ascending index, writes record k's key and seeds its box with itself.
// k_region_fill    the same blocks: a wavefront's 64 consecutive cells fall into runs of equal key; the run's first lane finds the region
//                  by binary search of the key in the field's ascending `first` column and adds the run's cells, sums and box (closed
//                  forms of the run's ends: region_run_sums) to the record -- in LDS for the block's own region (the first run's), which
//                  thread 0 carries to the record once, else by one set of global atomics per run, min / max only where they would
//                  change the word; all the run's lanes store the region's index.
// Registers and occupancy: DESIGN.md section 5.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcpp_regions.h"
#include "fcpp_regionfn.h"
#include "fcpp_samplefn.h"
#include "fcpp_launch.h"

namespace fcpp {

static constexpr int RBLOCK = 256;
static constexpr int RT = REGION_TILE;
static constexpr int RQ = RT * RT / RBLOCK;                     // cells per thread of a tile
static constexpr int RWAVE_CELLS = REGION_BLOCK_CELLS / (RBLOCK / 64);     // consecutive cells per wavefront of a numbering block
static constexpr int RROUNDS = RWAVE_CELLS / 64;

// a parent word, read or written while other lanes, wavefronts or workgroups do the same: relaxed atomics of the scope that shares it
template <int SCOPE>
__device__ __forceinline__ int32_t region_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE>
__device__ __forceinline__ void region_store(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }

// the root of member c.  Bounded: a parent is below its cell unless it is the cell itself, so the walk ends within c steps.
template <int SCOPE>
__device__ __forceinline__ int32_t region_find(const int32_t *P, int32_t c)
{
    int32_t p = region_load<SCOPE>(P + c);
    while (p != c) { c = p; p = region_load<SCOPE>(P + c); }
    return c;
}

// joins the sets of members a and b: the larger root takes the smaller as its parent.  Bounded: when the min finds that `a` had stopped
// being a root, the word it returns is below a (a parent of a, not a itself), and the next round starts from it: every retry strictly lowers
// a, and b never rises, so there are at most a retries.  The min has then hung a under min(old, b); joining old with b restores what it took.
template <int SCOPE>
__device__ __forceinline__ void region_union(int32_t *P, int32_t a, int32_t b)
{
    for (;;) {
        a = region_find<SCOPE>(P, a);
        b = region_find<SCOPE>(P, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

// the last field whose first tile / block is <= blk (a field without any shares its first with the next: never chosen); n >= 1
__device__ __forceinline__ int64_t region_field_of(const int64_t *__restrict__ first, int64_t n, int64_t blk)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {                                   // log2(n) rounds
        const int64_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(RBLOCK) void k_region_tiles(int64_t n, RegionFields F, const uint8_t *__restrict__ grid, int mask, int value,
                                                         int connectivity, int32_t *__restrict__ labels)
{
    __shared__ int32_t s_par[RT * RT];
    __shared__ unsigned long long s_row[RT];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = region_field_of(F.tile_first, n, blk);
    const RegionDims d = F.dims[f];
    const int64_t nx = d.nx, ny = d.ny, tiles_x = (nx + RT - 1) / RT;
    const int64_t tile = blk - F.tile_first[f], tx0 = (tile % tiles_x) * RT, ty0 = (tile / tiles_x) * RT;
    const int64_t at = F.cell_first[f], a = tx0 + lane;

    // ---- members: a row is one ballot; every member starts at the first cell of its horizontal run ----
    for (int q = 0; q < RQ; ++q) {
        const int y = wave + 4 * q;
        const int64_t b = ty0 + y;
        const bool m = a < nx && b < ny && region_member(grid[at + b * nx + a], mask, value);
        const unsigned long long row = __ballot(m);
        if (lane == 0) s_row[y] = row;
        const unsigned long long gaps = ~row & ((1ull << lane) - 1ull);       // the non-members left of this lane
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
        s_par[y * RT + lane] = m ? y * RT + start : -1;
    }
    __syncthreads();

    // ---- vertical links: the first cell of every overlap of this row's runs with the row above ----
    for (int q = 0; q < RQ; ++q) {
        const int y = wave + 4 * q;
        if (y == 0) continue;
        const unsigned long long row = s_row[y], up = s_row[y - 1], both = row & up;
        if (!((row >> lane) & 1ull)) continue;
        const int32_t c = y * RT + lane;
        if ((up >> lane) & 1ull) {
            // (the cell to the left, when it is a member under a member, is in this cell's run and under the same run above: it, or one further left, links)
            if (lane == 0 || !((both >> (lane - 1)) & 1ull)) region_union<WG>(s_par, c, c - RT);
        } else if (connectivity == 8) {                  // (with N a member, NW and NE lie in N's run)
            if (lane > 0 && ((up >> (lane - 1)) & 1ull)) region_union<WG>(s_par, c, c - RT - 1);
            if (lane < 63 && ((up >> (lane + 1)) & 1ull)) region_union<WG>(s_par, c, c - RT + 1);
        }
    }
    __syncthreads();

    // ---- every cell: the field-local index of its tile root (nobody writes s_par any more) ----
    if (a < nx) {
        for (int q = 0; q < RQ; ++q) {
            const int y = wave + 4 * q;
            const int64_t b = ty0 + y;
            if (b >= ny) break;
            const int32_t c = y * RT + lane;
            int32_t out = -1;
            if (s_par[c] >= 0) {
                const int32_t r = region_find<WG>(s_par, c);
                out = (int32_t)((ty0 + (r >> 6)) * nx + tx0 + (r & 63));
            }
            labels[at + b * nx + a] = out;
        }
    }
}

__global__ __launch_bounds__(RBLOCK) void k_region_seams(int64_t n, int64_t n_tiles, RegionFields F, int connectivity, int32_t *__restrict__ labels)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int64_t total = n_tiles * (2 * RT), stride = (int64_t)gridDim.x * RBLOCK;
    for (int64_t s = (int64_t)blockIdx.x * RBLOCK + threadIdx.x; s < total; s += stride) {      // ceil(total / stride) rounds
        const int64_t blk = s / (2 * RT);
        const int e = (int)(s % (2 * RT)), side = e >> 6, i = e & 63;
        const int64_t f = region_field_of(F.tile_first, n, blk);
        const RegionDims d = F.dims[f];
        const int64_t nx = d.nx, ny = d.ny, tiles_x = (nx + RT - 1) / RT;
        const int64_t tile = blk - F.tile_first[f], tx0 = (tile % tiles_x) * RT, ty0 = (tile / tiles_x) * RT;
        const int64_t a = side ? tx0 + i : tx0, b = side ? ty0 : ty0 + i;
        if (a >= nx || b >= ny) continue;
        int32_t *L = labels + F.cell_first[f];
        const int32_t c = (int32_t)(b * nx + a);
        if (region_load<AG>(L + c) < 0) continue;
        // across the seam: side 0 -> W, and under connectivity 8 NW and SW; side 1 -> N, and NW and NE
        const int nn = connectivity == 8 ? 3 : 1;
        for (int k = 0; k < nn; ++k) {
            const int64_t na = side ? a + (k == 0 ? 0 : k == 1 ? -1 : 1) : a - 1;
            const int64_t nb = side ? b - 1 : b + (k == 0 ? 0 : k == 1 ? -1 : 1);
            if (na < 0 || na >= nx || nb < 0 || nb >= ny) continue;
            const int32_t m = (int32_t)(nb * nx + na);
            if (region_load<AG>(L + m) >= 0) region_union<AG>(L, c, m);
        }
    }
}

template <bool FLATTEN>
__global__ __launch_bounds__(RBLOCK) void k_region_count(int64_t n, RegionFields F, int32_t *__restrict__ labels, int64_t *__restrict__ block_count)
{
    __shared__ int s_cnt[RBLOCK / 64];
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = region_field_of(F.block_first, n, blk);
    const int64_t nc = F.dims[f].nx * F.dims[f].ny;
    int32_t *L = labels + F.cell_first[f];
    const int64_t c0 = (blk - F.block_first[f]) * REGION_BLOCK_CELLS + (int64_t)wave * RWAVE_CELLS + lane;
    int cnt = 0;
    for (int k = 0; k < RROUNDS; ++k) {
        const int64_t c = c0 + 64 * k;
        if (c >= nc) break;
        int32_t p = FLATTEN ? region_load<AG>(L + c) : L[c];
        if (FLATTEN && p >= 0) {
            const int32_t r = region_find<AG>(L, (int32_t)c);
            if (r != p) region_store<AG>(L + c, r);
            p = r;
        }
        cnt += p == (int32_t)c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
        for (int w = 0; w < RBLOCK / 64; ++w) all += s_cnt[w];
        block_count[blk] = all;
    }
}

struct RegionBlockCount {
    const int64_t *count;
    __device__ int64_t operator()(int64_t p, int64_t &) const { return count[p]; }
};

__global__ __launch_bounds__(RBLOCK) void k_region_offsets(int64_t n, const int64_t *__restrict__ block_first, const int64_t *__restrict__ block_prefix,
                                                           int64_t *__restrict__ region_offsets)
{
    const int64_t i = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (i <= n) region_offsets[i] = block_prefix[block_first[i]];
}

__global__ __launch_bounds__(RBLOCK) void k_region_first(int64_t n, RegionFields F, const int32_t *__restrict__ labels,
                                                         const int64_t *__restrict__ block_prefix, const int64_t *__restrict__ region_offsets,
                                                         RegionRecord *__restrict__ records)
{
    __shared__ int s_cnt[RBLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = region_field_of(F.block_first, n, blk);
    const int64_t nx = F.dims[f].nx, nc = nx * F.dims[f].ny;
    const int32_t *L = labels + F.cell_first[f];
    const int64_t c0 = (blk - F.block_first[f]) * REGION_BLOCK_CELLS + (int64_t)wave * RWAVE_CELLS + lane;
    unsigned roots = 0;                                 // bit k: this lane's cell of round k is a root
    int mine = 0;                                       // the wavefront's roots
    for (int k = 0; k < RROUNDS; ++k) {
        const int64_t c = c0 + 64 * k;
        const bool root = c < nc && L[c] == (int32_t)c;
        roots |= root ? 1u << k : 0u;
        mine += __popcll(__ballot(root));
    }
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    int64_t at = region_offsets[f] + (block_prefix[blk] - block_prefix[F.block_first[f]]);
    for (int w = 0; w < wave; ++w) at += s_cnt[w];
    const int64_t end = region_offsets[f + 1];          // (labels that are not this call's keys must not write beside the field's records)
    for (int k = 0; k < RROUNDS; ++k) {
        const bool root = (roots >> k) & 1u;
        const unsigned long long m = __ballot(root);
        const int64_t slot = at + __popcll(m & ((1ull << lane) - 1ull));
        at += __popcll(m);
        if (root && slot < end) {
            const int64_t c = c0 + 64 * k;
            const int32_t ca = (int32_t)(c % nx), cb = (int32_t)(c / nx);
            records[slot] = { c, 0, ca, ca, cb, cb, 0, 0 };
        }
    }
}

// a run's, or a block's, cells, sums and box join a record: integer atomics, so the record does not depend on the order.  A box word only
// ever moves outwards: what lies inside the box that is there leaves it alone.
__device__ __forceinline__ void region_record_join(RegionRecord *R, unsigned long long cells, unsigned long long sum_a, unsigned long long sum_b,
                                                   int32_t a_min, int32_t a_max, int32_t b_min, int32_t b_max)
{
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    atomicAdd((unsigned long long *)&R->cells, cells);
    atomicAdd((unsigned long long *)&R->sum_a, sum_a);
    atomicAdd((unsigned long long *)&R->sum_b, sum_b);
    if (a_min < region_load<AG>(&R->a_min)) atomicMin(&R->a_min, a_min);
    if (a_max > region_load<AG>(&R->a_max)) atomicMax(&R->a_max, a_max);
    if (b_min < region_load<AG>(&R->b_min)) atomicMin(&R->b_min, b_min);
    if (b_max > region_load<AG>(&R->b_max)) atomicMax(&R->b_max, b_max);
}

__global__ __launch_bounds__(RBLOCK) void k_region_fill(int64_t n, RegionFields F, int32_t *__restrict__ labels, const int64_t *__restrict__ region_offsets,
                                                        RegionRecord *__restrict__ records)
{
    // the block's OWN region: the first run to claim the slot names it, and every run of that region in the block adds to LDS; thread 0
    // carries the sums to the record once.  (A large region spans thousands of blocks: one set of global atomics a block, not one a run.)
    __shared__ int32_t s_key, s_box[4];
    __shared__ unsigned long long s_sum[3];
    __shared__ int64_t s_rec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = region_field_of(F.block_first, n, blk);
    const int64_t nx = F.dims[f].nx, nc = nx * F.dims[f].ny;
    int32_t *L = labels + F.cell_first[f];
    const int64_t r0 = region_offsets[f], r1 = region_offsets[f + 1];
    if (tid == 0) {
        s_key = -1; s_rec = 0;
        s_box[0] = INT32_MAX; s_box[1] = -1; s_box[2] = INT32_MAX; s_box[3] = -1;
        s_sum[0] = s_sum[1] = s_sum[2] = 0ull;
    }
    __syncthreads();
    const int64_t c0 = (blk - F.block_first[f]) * REGION_BLOCK_CELLS + (int64_t)wave * RWAVE_CELLS + lane;
    for (int k = 0; k < RROUNDS; ++k) {
        const int64_t c = c0 + 64 * k;
        if (c - lane >= nc) break;                      // (the whole wavefront: the shuffles below need every lane)
        const int32_t key = c < nc ? L[c] : -1;
        const int32_t prev = __shfl_up(key, 1);
        const bool differs = lane > 0 && prev != key;
        const bool head = key >= 0 && (lane == 0 || differs);
        const unsigned long long heads = __ballot(head), cuts = __ballot(differs);
        int32_t index = -1;
        if (head) {
            const unsigned long long above = lane == 63 ? 0ull : cuts & ~((2ull << lane) - 1ull);
            const int last = above ? __ffsll((long long)above) - 2 : 63;       // the run ends before the next lane that differs
            int64_t lo = r0, hi = r1;                   // the last record of the field whose key is <= this one: log2(regions) rounds
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (records[mid].first <= (int64_t)key) lo = mid; else hi = mid;
            }
            if (hi > lo && records[lo].first == (int64_t)key) {
                RegionRecord *R = records + lo;
                const int64_t c1 = c + (last - lane);
                int64_t sum_a, sum_b;
                int32_t a_min, a_max;
                region_run_sums(c, c1, nx, sum_a, sum_b);
                region_run_columns(c, c1, nx, a_min, a_max);
                const int32_t b_min = (int32_t)(c / nx), b_max = (int32_t)(c1 / nx);
                int32_t owner = region_load<__HIP_MEMORY_SCOPE_WORKGROUP>(&s_key);
                if (owner < 0) {
                    owner = atomicCAS(&s_key, -1, key);
                    if (owner < 0) { owner = key; s_rec = lo; }        // (claimed: read by thread 0 behind the barrier)
                }
                if (owner == key) {
                    atomicAdd(&s_sum[0], (unsigned long long)(c1 - c + 1));
                    atomicAdd(&s_sum[1], (unsigned long long)sum_a);
                    atomicAdd(&s_sum[2], (unsigned long long)sum_b);
                    atomicMin(&s_box[0], a_min); atomicMax(&s_box[1], a_max);
                    atomicMin(&s_box[2], b_min); atomicMax(&s_box[3], b_max);
                } else
                    region_record_join(R, (unsigned long long)(c1 - c + 1), (unsigned long long)sum_a, (unsigned long long)sum_b, a_min, a_max, b_min,
                                       b_max);
                index = (int32_t)(lo - r0);
            }
        }
        const unsigned long long below = heads & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
        const int from = below ? 63 - __clzll((long long)below) : lane;        // this lane's run starts there
        index = __shfl(index, from);
        if (key >= 0) L[c] = index;
    }
    __syncthreads();
    if (tid == 0 && s_key >= 0) region_record_join(records + s_rec, s_sum[0], s_sum[1], s_sum[2], s_box[0], s_box[1], s_box[2], s_box[3]);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_region_tiles(hipStream_t st, int64_t n, int64_t n_tiles, const RegionFields &f, const uint8_t *grid, int mask, int value,
                        int connectivity, int32_t *labels)
{
    if (n <= 0 || n_tiles <= 0) return 0;
    return launch(st, k_region_tiles, (unsigned)n_tiles, RBLOCK, n, f, grid, mask, value, connectivity, labels);
}

int launch_region_seams(hipStream_t st, int64_t n, int64_t n_tiles, const RegionFields &f, int connectivity, int32_t *labels, int max_blocks)
{
    if (n <= 0 || n_tiles <= 0) return 0;
    const int64_t need = (n_tiles * (2 * RT) + RBLOCK - 1) / RBLOCK;
    const int64_t blocks = need < (int64_t)max_blocks ? need : (int64_t)max_blocks;
    return launch(st, k_region_seams, (unsigned)(blocks > 0 ? blocks : 1), RBLOCK, n, n_tiles, f, connectivity, labels);
}

int launch_region_count(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, int flatten, int32_t *labels, int64_t *block_count)
{
    if (n <= 0 || n_blocks <= 0) return 0;
    return launch(st, flatten ? k_region_count<true> : k_region_count<false>, (unsigned)n_blocks, RBLOCK, n, f, labels, block_count);
}

int launch_region_offsets(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, const int64_t *block_count, int64_t *block_prefix,
                          int64_t *err, int64_t *region_offsets)
{
    if (int e = launch_path_counts<RBLOCK>(st, n_blocks, RegionBlockCount{ block_count }, block_prefix, err)) return e;
    if (region_offsets) {
        if (int e = launch(st, k_region_offsets, blocks_for(n + 1, RBLOCK), RBLOCK, n, f.block_first, block_prefix, region_offsets)) return e;
    }
    return 0;
}

int launch_region_first(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, const int32_t *labels, const int64_t *block_prefix,
                        const int64_t *region_offsets, RegionRecord *records)
{
    if (n <= 0 || n_blocks <= 0) return 0;
    return launch(st, k_region_first, (unsigned)n_blocks, RBLOCK, n, f, labels, block_prefix, region_offsets, records);
}

int launch_region_fill(hipStream_t st, int64_t n, int64_t n_blocks, const RegionFields &f, int32_t *labels, const int64_t *region_offsets,
                       RegionRecord *records)
{
    if (n <= 0 || n_blocks <= 0) return 0;
    return launch(st, k_region_fill, (unsigned)n_blocks, RBLOCK, n, f, labels, region_offsets, records);
}

}  // namespace fcpp
