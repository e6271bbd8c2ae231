// fcpp_patch.hip -- gfx950 (MI355X) kernels of the patch passes (include/fcpp.h: fcpp_patch_sizes, fcpp_patch_counts, fcpp_patch_fill):
// straight working passes over the member cells of labelled coverage regions.  The rule is fcpp_patchfn.h: extents are exact min / max,
// everything behind a member's two `floor`s is integer work, so the kernels give what fcpp_debug_patch_swaths gives on the host, whatever
// the order the hardware works in.  Plain C++: no inline assembly, vector integer atomics only (max, or), no spin waits, every loop bounded.
//
// The cells are walked as k_region_fill walks them: a workgroup of 256 per numbering block (4096 consecutive cells of ONE field), a
// wavefront per 1024, 64 consecutive cells a round.
//
// k_patch_frame    a lane per field: (s, c) = fc_sincos(theta).
// k_patch_extent   the 64 cells of a round fall into runs of equal label; a run reduces the keys of -u, u, -w, w (patch_key: they order as
//                  the doubles do) by a segmented max in the wave, and its first lane joins them to the first four words of the region's
//                  record by 64-bit integer atomic max -- only where the word would change.  No float atomics: nothing depends on the order.
// k_patch_layout   ONE workgroup: a lane per region turns the keys into the record (patch_layout: K, B, w_lo, status) inside the samplers'
//                  scan (fcpp_samplefn.h, as it is) of the lines, a second scan of the bitmap words; then every record takes its first
//                  line and first word.
// k_patch_mark     the same walk: a member's word and bit from its line and bin; adjacent lanes that hit the same word OR their bits in
//                  the wave, then one atomic OR per word -- only where the word would change.
// k_patch_runs     a wavefront per line, a lane per 64-bin word, in rounds of 64 words; at most `max_blocks` workgroups stride over the
//                  lines.  The last set bin before a lane's word is an exclusive prefix max across the wave, carried from round to round;
//                  a start is a set bin more than J bins behind the previous set bin.  FILL = 0 counts the starts.  FILL = 1: start
//                  number t writes record t's first end, line and region and closes record t - 1 (its second end at the previous set
//                  bin, its length from the previous start, likewise a carried prefix max); lane 0 closes the line's last record.
// k_patch_offsets  the swaths before every field's first line, from the scan of the lines' counts.
// Registers and occupancy: DESIGN.md section 5.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcpp_launch.h"
#include "fcpp_patch.h"
#include "fcpp_patchfn.h"
#include "fcpp_samplefn.h"

namespace fcpp {

static constexpr int PBLOCK = 256;
static constexpr int PWAVES = PBLOCK / 64;
static constexpr int PWAVE_CELLS = REGION_BLOCK_CELLS / PWAVES;            // consecutive cells per wavefront of a numbering block
static constexpr int PROUNDS = PWAVE_CELLS / 64;
typedef unsigned long long u64;

__device__ __forceinline__ u64 patch_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the run of equal `key` this lane lies in among the wave's 64 lanes: is this lane its first, and which lane is its last
__device__ __forceinline__ void patch_lane_run(int64_t key, int lane, bool &first, int &last)
{
    const int64_t prev = __shfl_up(key, 1);
    const bool differs = lane > 0 && prev != key;
    const u64 cuts = __ballot(differs);
    const u64 above = lane == 63 ? 0ull : cuts & ~((2ull << lane) - 1ull);
    last = above ? __ffsll((long long)above) - 2 : 63;          // the run ends before the next lane that differs
    first = lane == 0 || differs;
}

// a member's cell of this round: its label within 0 .. n_reg - 1, else -1
__device__ __forceinline__ int32_t patch_label(const int32_t *__restrict__ L, int64_t c, int64_t nc, int64_t n_reg)
{
    const int32_t lab = c < nc ? L[c] : -1;
    return lab >= 0 && (int64_t)lab < n_reg ? lab : -1;
}

__global__ __launch_bounds__(PBLOCK) void k_patch_frame(int64_t n, const double *__restrict__ angle, double *__restrict__ frame)
{
    const int64_t i = (int64_t)blockIdx.x * PBLOCK + threadIdx.x;
    if (i >= n) return;
    double s, c;
    fc_sincos(angle[i], s, c);
    frame[2 * i] = s; frame[2 * i + 1] = c;
}

__global__ __launch_bounds__(PBLOCK) void k_patch_extent(int64_t n, PatchFields F, PatchRule rule, const int32_t *__restrict__ labels,
                                                         PatchRecord *__restrict__ records)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = last_at_or_before(n, blk, [&](int64_t i) { return F.block_first[i]; });
    const uint32_t nx = (uint32_t)F.dims[f].nx;
    const int64_t nc = (int64_t)nx * F.dims[f].ny;
    const int32_t *L = labels + F.cell_first[f];
    const int64_t r0 = F.region_first[f], n_reg = F.region_first[f + 1] - r0;
    const double s = F.frame[2 * f], c = F.frame[2 * f + 1];
    const int64_t c0 = (blk - F.block_first[f]) * REGION_BLOCK_CELLS + (int64_t)wave * PWAVE_CELLS + lane;
    for (int k = 0; k < PROUNDS; ++k) {
        const int64_t cell = c0 + 64 * k;
        if (cell - lane >= nc) break;                   // (the whole wavefront: the shuffles below need every lane)
        const int32_t lab = patch_label(L, cell, nc, n_reg);
        if (__ballot(lab >= 0) == 0ull) continue;       // (the whole wavefront: most rounds of a planned field hold no member)
        bool first;
        int last;
        patch_lane_run(lab, lane, first, last);
        u64 v[4] = { 0ull, 0ull, 0ull, 0ull };
        if (lab >= 0) {
            double u, w;
            patch_cell_uw((int64_t)((uint32_t)cell % nx), (int64_t)((uint32_t)cell / nx), rule.res, c, s, u, w);
            v[0] = patch_key(-u); v[1] = patch_key(u); v[2] = patch_key(-w); v[3] = patch_key(w);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u64 t = __shfl_down(v[j], o);
                if (lane + o <= last && t > v[j]) v[j] = t;
            }
        if (first && lab >= 0) {
            u64 *R = (u64 *)(records + r0 + lab);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v[j] > patch_load(R + j)) atomicMax(R + j, v[j]);
        }
    }
}

__global__ __launch_bounds__(PBLOCK) void k_patch_layout(int64_t n_regions, PatchRule rule, PatchRecord *__restrict__ records,
                                                         int64_t *__restrict__ line_first, int64_t *__restrict__ word_first, int64_t *__restrict__ err)
{
    // ---- the layout of every region, and the lines before it ----
    sample_scan<PBLOCK>(n_regions, [=](int64_t p, int64_t &) {
        const u64 *R = (const u64 *)(records + p);
        const PatchRecord r = patch_layout(R[0], R[1], R[2], R[3], rule.We, rule.res);
        records[p] = r;
        return r.K;
    }, line_first, err);
    // ---- the bitmap words before it (every lane reads the records it wrote itself) ----
    sample_scan<PBLOCK>(n_regions, [=](int64_t p, int64_t &) { return records[p].K * patch_words_per_line(records[p].B); }, word_first, err);
    // ---- every record takes its place (the scans' entries p are this lane's own stores) ----
    for (int64_t p = threadIdx.x; p < n_regions; p += PBLOCK) {         // ceil(n_regions / 256) rounds
        records[p].first_line = line_first[p];
        records[p].first_word = word_first[p];
    }
}

__global__ __launch_bounds__(PBLOCK) void k_patch_mark(int64_t n, PatchFields F, PatchRule rule, const int32_t *__restrict__ labels,
                                                       const PatchRecord *__restrict__ records, int64_t n_words, u64 *__restrict__ bitmap)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const int64_t f = last_at_or_before(n, blk, [&](int64_t i) { return F.block_first[i]; });
    const uint32_t nx = (uint32_t)F.dims[f].nx;
    const int64_t nc = (int64_t)nx * F.dims[f].ny;
    const int32_t *L = labels + F.cell_first[f];
    const int64_t r0 = F.region_first[f], n_reg = F.region_first[f + 1] - r0;
    const double s = F.frame[2 * f], c = F.frame[2 * f + 1];
    const int64_t c0 = (blk - F.block_first[f]) * REGION_BLOCK_CELLS + (int64_t)wave * PWAVE_CELLS + lane;
    for (int k = 0; k < PROUNDS; ++k) {
        const int64_t cell = c0 + 64 * k;
        if (cell - lane >= nc) break;                   // (the whole wavefront)
        const int32_t lab = patch_label(L, cell, nc, n_reg);
        if (__ballot(lab >= 0) == 0ull) continue;       // (the whole wavefront)
        int64_t word = -1;
        u64 bits = 0ull;
        if (lab >= 0) {
            const PatchRecord *R = records + r0 + lab;
            const int64_t K = R->K, B = R->B;
            if (K > 0 && B > 0) {
                double u, w;
                patch_cell_uw((int64_t)((uint32_t)cell % nx), (int64_t)((uint32_t)cell / nx), rule.res, c, s, u, w);
                const int64_t ln = patch_line(w, R->w_lo, rule.We, K), q = patch_bin(u, R->u_min, rule.res, B);
                word = R->first_word + ln * patch_words_per_line(B) + (q >> 6);
                bits = 1ull << (q & 63);
                if (word < 0 || word >= n_words) { word = -1; bits = 0ull; }        // (records that are not this call's must not write beside the bitmap)
            }
        }
        bool first;
        int last;
        patch_lane_run(word, lane, first, last);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = __shfl_down(bits, o);
            if (lane + o <= last) bits |= t;
        }
        if (first && word >= 0 && (patch_load(bitmap + word) & bits) != bits) atomicOr(bitmap + word, bits);
    }
}

// an inclusive prefix max over the wave's lanes
__device__ __forceinline__ int64_t patch_scan_max(int64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(v, o);
        if (lane >= o && t > v) v = t;
    }
    return v;
}

// what lies before this lane: the inclusive scan `inc` of the lanes below, and `carry` of the rounds before
__device__ __forceinline__ int64_t patch_before(int64_t inc, int64_t carry, int lane)
{
    const int64_t below = __shfl_up(inc, 1);
    return lane == 0 || carry > below ? carry : below;
}

template <bool FILL>
__global__ __launch_bounds__(PBLOCK) void k_patch_runs(int64_t n, int64_t n_regions, int64_t n_lines, int64_t n_words, PatchFields F, PatchRule rule,
                                                       const PatchRecord *__restrict__ records, const u64 *__restrict__ bitmap,
                                                       int64_t *__restrict__ line_counts, const int64_t *__restrict__ line_offsets, PatchSwaths out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * PWAVES;
    for (int64_t line = (int64_t)blockIdx.x * PWAVES + wave; line < n_lines; line += stride) {          // ceil(n_lines / stride) rounds, a wavefront's lanes together
        const int64_t r = last_at_or_before(n_regions, line, [&](int64_t i) { return records[i].first_line; });
        const PatchRecord R = records[r];
        const int64_t k = line - R.first_line;
        const int64_t wpl = R.B > 0 && R.B <= PATCH_MAX_JOIN_BINS ? patch_words_per_line(R.B) : 0;
        // (records that are not this call's must not read beside the bitmap)
        const bool ok = R.K > 0 && R.K <= PATCH_MAX_LINES && k >= 0 && k < R.K && wpl > 0 && R.first_word >= 0 && R.first_word <= n_words
                        && (k + 1) * wpl <= n_words - R.first_word;
        if (!ok) {
            if (!FILL && lane == 0) line_counts[line] = 0;
            continue;
        }
        const u64 *words = bitmap + R.first_word + k * wpl;
        // FILL: where the line's records go and what they share
        int64_t base = 0, end = 0, f = 0;
        double s = 0.0, c = 1.0, gx = 0.0, gy = 0.0, wk = 0.0;
        int32_t line_in_field = 0;
        if (FILL) {
            f = last_at_or_before(n, r, [&](int64_t i) { return F.region_first[i]; });
            s = F.frame[2 * f]; c = F.frame[2 * f + 1];
            gx = F.dims[f].gx; gy = F.dims[f].gy;
            wk = patch_line_w(R.w_lo, rule.We, k);
            line_in_field = (int32_t)(line - records[F.region_first[f]].first_line);
            base = line_offsets[line]; end = line_offsets[line + 1];
            if (end > out.n_swaths) end = out.n_swaths;
            if (base < 0) base = end;
        }
        auto close = [&](int64_t t, int64_t q0, int64_t q1) {          // record t of the line: its second end and its length
            const int64_t at = base + t;
            if (at >= end || q0 < 0 || q1 < 0) return;
            const double ua = patch_u_a(R.u_min, rule.res, rule.m, q0), ub = patch_u_b(R.u_min, rule.res, rule.m, q1);
            double x, y;
            patch_end_point(ub, wk, c, s, gx, gy, x, y);
            out.bx[at] = x; out.by[at] = y; out.length[at] = ub - ua;
        };
        int64_t last_set = -1, last_start = -1, starts = 0;          // of the rounds before
        for (int64_t w0 = 0; w0 < wpl; w0 += 64) {          // ceil(wpl / 64) rounds
            const int64_t wi = w0 + lane;
            const u64 bits = wi < wpl ? words[wi] : 0ull;
            const int64_t set_inc = patch_scan_max(bits ? wi * 64 + 63 - __clzll((long long)bits) : -1, lane);
            const int64_t set_before = patch_before(set_inc, last_set, lane);
            // a bit behind a set bit of its own word never starts a run: the others ask their previous set bin
            const u64 cand = bits & ~(bits << 1);
            int cnt = 0;
            int64_t my_start = -1;
            for (u64 m = cand; m; m &= m - 1ull) {          // at most 32 rounds
                const int j = __ffsll((long long)m) - 1;
                const u64 below = bits & ((1ull << j) - 1ull);
                const int64_t prev = below ? wi * 64 + 63 - __clzll((long long)below) : set_before;
                if (patch_starts(wi * 64 + j, prev, rule.J)) { ++cnt; my_start = wi * 64 + j; }
            }
            int cnt_inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(cnt_inc, o);
                if (lane >= o) cnt_inc += t;
            }
            if (FILL) {
                const int64_t start_inc = patch_scan_max(my_start, lane);
                int64_t q0 = patch_before(start_inc, last_start, lane);          // the start of the run that is open
                int64_t t = starts + cnt_inc - cnt;
                for (u64 m = cand; m; m &= m - 1ull) {
                    const int j = __ffsll((long long)m) - 1;
                    const u64 below = bits & ((1ull << j) - 1ull);
                    const int64_t q = wi * 64 + j, prev = below ? wi * 64 + 63 - __clzll((long long)below) : set_before;
                    if (!patch_starts(q, prev, rule.J)) continue;
                    if (t > 0) close(t - 1, q0, prev);
                    const int64_t at = base + t;
                    if (at < end) {
                        double x, y;
                        patch_end_point(patch_u_a(R.u_min, rule.res, rule.m, q), wk, c, s, gx, gy, x, y);
                        out.ax[at] = x; out.ay[at] = y; out.line[at] = line_in_field; out.region[at] = r;
                    }
                    q0 = q; ++t;
                }
                const int64_t round_start = __shfl(start_inc, 63);
                if (round_start > last_start) last_start = round_start;
            }
            const int64_t round_set = __shfl(set_inc, 63);
            if (round_set > last_set) last_set = round_set;
            starts += __shfl(cnt_inc, 63);
        }
        if (!FILL) {
            if (lane == 0) line_counts[line] = starts;
        } else if (lane == 0 && starts > 0) close(starts - 1, last_start, last_set);
    }
}

struct PatchLineCount {
    const int64_t *count;
    __device__ int64_t operator()(int64_t p, int64_t &) const { return count[p]; }
};

__global__ __launch_bounds__(PBLOCK) void k_patch_offsets(int64_t n, int64_t n_regions, int64_t n_lines, const int64_t *__restrict__ region_first,
                                                          const PatchRecord *__restrict__ records, const int64_t *__restrict__ line_offsets,
                                                          int64_t *__restrict__ swath_offsets)
{
    const int64_t i = (int64_t)blockIdx.x * PBLOCK + threadIdx.x;
    if (i > n) return;
    const int64_t r = region_first[i];
    int64_t l = r >= 0 && r < n_regions ? records[r].first_line : n_lines;
    if (l < 0 || l > n_lines) l = n_lines;
    swath_offsets[i] = line_offsets[l];
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int launch_patch_frame(hipStream_t st, int64_t n, const double *angle, double *frame)
{
    if (n <= 0) return 0;
    return launch(st, k_patch_frame, blocks_for(n, PBLOCK), PBLOCK, n, angle, frame);
}

int launch_patch_extent(hipStream_t st, int64_t n, int64_t n_blocks, const PatchFields &f, const PatchRule &rule, const int32_t *labels,
                        PatchRecord *records)
{
    if (n <= 0 || n_blocks <= 0) return 0;
    return launch(st, k_patch_extent, (unsigned)n_blocks, PBLOCK, n, f, rule, labels, records);
}

int launch_patch_layout(hipStream_t st, int64_t n_regions, const PatchRule &rule, PatchRecord *records, int64_t *line_first, int64_t *word_first,
                        int64_t *err)
{
    return launch(st, k_patch_layout, 1, PBLOCK, n_regions, rule, records, line_first, word_first, err);
}

int launch_patch_mark(hipStream_t st, int64_t n, int64_t n_blocks, const PatchFields &f, const PatchRule &rule, const int32_t *labels,
                      const PatchRecord *records, int64_t n_words, unsigned long long *bitmap)
{
    if (n <= 0 || n_blocks <= 0 || n_words <= 0) return 0;
    return launch(st, k_patch_mark, (unsigned)n_blocks, PBLOCK, n, f, rule, labels, records, n_words, bitmap);
}

int launch_patch_runs(hipStream_t st, int fill, int64_t n, int64_t n_regions, int64_t n_lines, int64_t n_words, const PatchFields &f,
                      const PatchRule &rule, const PatchRecord *records, const unsigned long long *bitmap, int64_t *line_counts,
                      const int64_t *line_offsets, const PatchSwaths &out, int max_blocks)
{
    if (n <= 0 || n_regions <= 0 || n_lines <= 0) return 0;
    const int64_t need = (n_lines + PWAVES - 1) / PWAVES;
    const int64_t blocks = need < (int64_t)max_blocks ? need : (int64_t)max_blocks;
    return launch(st, fill ? k_patch_runs<true> : k_patch_runs<false>, (unsigned)(blocks > 0 ? blocks : 1), PBLOCK, n, n_regions, n_lines, n_words, f,
                  rule, records, bitmap, line_counts, line_offsets, out);
}

int launch_patch_offsets(hipStream_t st, int64_t n, int64_t n_regions, int64_t n_lines, const PatchFields &f, const PatchRecord *records,
                         const int64_t *line_counts, int64_t *line_offsets, int64_t *err, int64_t *swath_offsets)
{
    if (int e = launch_path_counts<PBLOCK>(st, n_lines, PatchLineCount{ line_counts }, line_offsets, err)) return e;
    return launch(st, k_patch_offsets, blocks_for(n + 1, PBLOCK), PBLOCK, n, n_regions, n_lines, f.region_first, records, line_offsets,
                  swath_offsets);
}

}  // namespace fcpp
