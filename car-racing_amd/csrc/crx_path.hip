// crx_path.hip -- the 1-D QPs of the overtake PATH planner:
//   crx_path_kernel   crx_path_qp.h without a mask: every QP of the batch is solved (crx_path_solve[_dev])
// Restates planning/overtake_path_planner.py:199-318 of the reference (the text and its description: crx_path_qp.h).
// The masked instantiation, crx_path_masked_kernel, is crx_pathplan.hip's; crx_path_qp.h says why the two do not share a unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crx_kparams.h"
#include "crx_wave.h"
#include "crx_ipm.h"

#define CRX_PATH_KERNEL crx_path_kernel
#define CRX_PATH_KPARAMS crx_path_kparams
#define CRX_PATH_SKIP(pp, b, lane)
#include "crx_path_qp.h"

hipError_t crx_launch_path(const crx_path_kparams& pp, hipStream_t st) { return crx_launch_1d(crx_path_kernel, pp.batch, 1, WAVE, st, pp); }
