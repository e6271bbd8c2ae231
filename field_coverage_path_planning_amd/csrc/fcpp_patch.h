// fcpp_patch.h -- interface between the C-ABI glue (fcpp_glue_cover.cpp) and the patch-pass kernels (fcpp_patch.hip): the regions' extents and
// layout, the bitmaps of their lines, the runs of every line and the swath records.  The rule is fcpp_patchfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_patchfn.h"

namespace fcpp {

// the fields of a call, device pointers: the caller's grids, labels' regions and frame, and where the glue's checked table places the
// numbering blocks (REGION_BLOCK_CELLS consecutive cells of one field)
struct PatchFields {
    const RegionDims *dims;                      // n
    const int64_t *cell_first;                   // n + 1: the caller's cell_offsets
    const int64_t *block_first;                  // n + 1
    const int64_t *region_first;                 // n + 1: the caller's region_offsets
    const double *frame;                         // n x 2: s, c
};

// what the rule takes besides the fields
struct PatchRule {
    double res, We, m;
    int64_t J;
};

// where fcpp_patch_fill writes: m records, SoA
struct PatchSwaths {
    double *ax, *ay, *bx, *by, *length;
    int32_t *line;
    int64_t *region;
    int64_t n_swaths;
};

// every launcher returns 0 or a hipError_t value
// frame (n x 2) = fc_sincos of the fields' angles
int launch_patch_frame(hipStream_t st, int64_t n, const double *angle, double *frame);
// a workgroup per numbering block: the members' keys join the first four words of their regions' records (zeroed before)
int launch_patch_extent(hipStream_t st, int64_t n, int64_t n_blocks, const PatchFields &f, const PatchRule &rule, const int32_t *labels,
                        PatchRecord *records);
// one workgroup: every region's layout from its keys, then first line and first word by the samplers' scan; line_first, word_first:
// n_regions + 1 words of scratch each (their last entries are the call's totals), err: one word
int launch_patch_layout(hipStream_t st, int64_t n_regions, const PatchRule &rule, PatchRecord *records, int64_t *line_first, int64_t *word_first,
                        int64_t *err);
// a workgroup per numbering block: the members set their bits (bitmap zeroed before)
int launch_patch_mark(hipStream_t st, int64_t n, int64_t n_blocks, const PatchFields &f, const PatchRule &rule, const int32_t *labels,
                      const PatchRecord *records, int64_t n_words, unsigned long long *bitmap);
// a wavefront per line, at most max_blocks workgroups stride over the lines.  fill == 0: line_counts[line] = its runs; fill != 0: the
// swath records of every line, from line_offsets (n_lines + 1)
int launch_patch_runs(hipStream_t st, int fill, int64_t n, int64_t n_regions, int64_t n_lines, int64_t n_words, const PatchFields &f,
                      const PatchRule &rule, const PatchRecord *records, const unsigned long long *bitmap, int64_t *line_counts,
                      const int64_t *line_offsets, const PatchSwaths &out, int max_blocks);
// line_offsets (n_lines + 1) = the exclusive scan of line_counts (the samplers' scan; err: one word of scratch), swath_offsets (n + 1) =
// the swaths before every field's first line
int launch_patch_offsets(hipStream_t st, int64_t n, int64_t n_regions, int64_t n_lines, const PatchFields &f, const PatchRecord *records,
                         const int64_t *line_counts, int64_t *line_offsets, int64_t *err, int64_t *swath_offsets);

}  // namespace fcpp
