// fcpp_mission.h -- interface between the C-ABI glue (fcpp_glue_mission.cpp) and the mission-path kernels (fcpp_mission.hip).  The rule is
// fcpp_missionfn.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "fcpp_missionfn.h"

namespace fcpp {

constexpr int MISSION_BLOCK = 256;                       // threads of a workgroup of every kernel: four wavefronts, a target node each

// every launcher returns 0 or a hipError_t value.  `in` holds device pointers whose offsets and item_path the caller has checked.
// a wavefront per item: its nodes in order (T.st_idx) and their number (T.n_nodes)
int launch_mission_stations(hipStream_t st, const MissionIn &in, const MissionTemp &T);
// Solve pass, a workgroup per field: T.pred of every node and T.end_node
int launch_mission_layers(hipStream_t st, int mode, const MissionIn &in, const MissionTemp &T);
// a lane per field: mission_finish
int launch_mission_finish(hipStream_t st, int mode, const MissionIn &in, const MissionTemp &T, const MissionOut &out);
// the scan of the slots' sample counts (fcpp_samplefn.h) into slot_offsets (n_slots + 1), the fields' ends of it into path_offsets
// (n_fields + 1); err[0]: the slots of 2^31 - 1 samples or more
int launch_mission_counts(hipStream_t st, int mode, const MissionIn &in, const MissionRec &rec, double spacing, int64_t *slot_offsets,
                          int64_t *path_offsets, int64_t *err);
// a lane per output sample; every output may be NULL
int launch_mission_fill(hipStream_t st, int mode, const MissionIn &in, const MissionRec &rec, double spacing, const int64_t *slot_offsets,
                        int64_t total_samples, double *x, double *y, double *heading, double *kappa, int8_t *part, int8_t *gear, int32_t *slot,
                        int64_t *src);

}  // namespace fcpp
