// crx_plant.hip -- the plant, the four inclusions of crx_plant_step.h:
//   crx_plant_kernel              one control step of the plant for a batch of vehicles, one BicycleDynamicsParam set for the launch
//   crx_plant_cars_kernel         the same step with one BicycleDynamicsParam set per vehicle (params[batch][10])
//   crx_plant_tracks_kernel       the same step with car b on track track_id[b] of a track set, the descriptor's BicycleDynamicsParam set
//   crx_plant_tracks_cars_kernel  car b on its own track with its own BicycleDynamicsParam set
//
// ------------------------------------------------------------------------------------------------
// Plant: one thread per vehicle, n_sub Euler sub-steps.  Restates
//   system/vehicle_dynamics.py:4-49          one Euler step, global + curvilinear
//   utils/racing_env.py:225-246              curvature lookup (first matching segment, inclusive ends)
//   utils/base.py:897-942                    DynamicBicycleModel.forward_dynamics, zero noise
// Compute-bound on transcendentals (2 atan2, 2 atan, 6 sin/cos per sub-step); HBM traffic 14+12 doubles
// per vehicle per control step.
// ------------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "crx_kparams.h"
#include "crx_wave.h"

// The step is written once, in crx_plant_step.h.  crx_plant_kernel: the ten BicycleDynamicsParam values are the descriptor's, uniform over the
// launch.  crx_plant_cars_kernel (crx_plant_step_params_dev): car b's own row params[10 b ..], in the order of BicycleDynamicsParam.get_params()
// (m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br), read into registers before the sub-step loop.  Everything else comes from the descriptor either way.
#define CRX_PLANT_PARAMS_DESC(pk, b)
#define CRX_PLANT_P_DESC(name) d.name
#define CRX_PLANT_PARAMS_CARS(pk, b)                                                                                                  \
    const double* row = pk.params + CRX_PLANT_NPARAM * (size_t)b;                                                                     \
    const double car_m = row[0], car_lf = row[1], car_lr = row[2], car_Iz = row[3], car_Df = row[4], car_Cf = row[5], car_Bf = row[6], \
                 car_Dr = row[7], car_Cr = row[8], car_Br = row[9];
#define CRX_PLANT_P_CARS(name) car_##name

// One table for the launch: the block stages the descriptor's n_seg rows, every lane scans all of them (LDS broadcasts) and wraps at the
// descriptor's lap length.
#define CRX_PLANT_TABLES_ONE(pk)                                                                          \
    __shared__ double seg_lo[CRX_PLANT_MAX_SEG], seg_hi[CRX_PLANT_MAX_SEG], seg_cv[CRX_PLANT_MAX_SEG];    \
    const crx_plant_desc& d = pk.d;                                                                       \
    for (int i = threadIdx.x; i < d.n_seg; i += blockDim.x) {                                             \
        seg_lo[i] = pk.track[6 * i + 3];                                                                  \
        seg_hi[i] = pk.track[6 * i + 3] + pk.track[6 * i + 4];                                            \
        seg_cv[i] = pk.track[6 * i + 5];                                                                  \
    }                                                                                                     \
    __syncthreads();
#define CRX_PLANT_TRACK_ONE(pk, b)
#define CRX_PLANT_NSEG_ONE d.n_seg
#define CRX_PLANT_ROW_ONE(a, i) a[i]
#define CRX_PLANT_LAP_ONE d.lap_length

// A track set (crx_plant_step_tracks_dev): the block stages all n_tracks * seg_stride rows, padding included, at their own index; car b scans
// the n_seg[t] rows from t * seg_stride on of its track t = track_id[b] (per-lane LDS reads) and wraps at lap_length[t].  What lives on the
// device cannot be validated on the host: a track_id outside [0, n_tracks) never becomes an address -- the car's two rows get NaN, its lap
// counter stays, and the lane leaves (after the block's only barrier); n_seg[t] is clamped to [0, seg_stride], so the scan stays inside the
// track's own rows whatever the array holds.
#define CRX_PLANT_TABLES_SET(pk)                                                                                                                  \
    __shared__ double seg_lo[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_hi[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG], seg_cv[CRX_MAX_TRACKS * CRX_PLANT_MAX_SEG]; \
    const crx_plant_desc& d = pk.d;                                                                                                               \
    for (int i = threadIdx.x; i < pk.n_tracks * pk.seg_stride; i += blockDim.x) {                                                                 \
        seg_lo[i] = pk.track[6 * i + 3];                                                                                                          \
        seg_hi[i] = pk.track[6 * i + 3] + pk.track[6 * i + 4];                                                                                    \
        seg_cv[i] = pk.track[6 * i + 5];                                                                                                          \
    }                                                                                                                                             \
    __syncthreads();
#define CRX_PLANT_TRACK_SET(pk, b)                                                                            \
    const int car_track = pk.track_id[b];                                                                     \
    if (car_track < 0 || car_track >= pk.n_tracks) {                                                          \
        for (int k = 0; k < 6; k++) { pk.xglob_next[6 * (size_t)b + k] = NAN; pk.xcurv_next[6 * (size_t)b + k] = NAN; } \
        return;                                                                                               \
    }                                                                                                         \
    const int car_row0 = car_track * pk.seg_stride, car_nseg = min(max(pk.n_seg[car_track], 0), pk.seg_stride); \
    const double car_lap = pk.lap_length[car_track];
#define CRX_PLANT_NSEG_SET car_nseg
#define CRX_PLANT_ROW_SET(a, i) a[car_row0 + i]
#define CRX_PLANT_LAP_SET car_lap

// one inclusion: the kernel, its parameter struct, the parameter source (DESC / CARS) and the track source (ONE / SET)
#define CRX_PLANT_KERNEL crx_plant_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams
#define CRX_PLANT_READ_PARAMS(pk, b) CRX_PLANT_PARAMS_DESC(pk, b)
#define CRX_PLANT_P(name) CRX_PLANT_P_DESC(name)
#define CRX_PLANT_TABLES(pk) CRX_PLANT_TABLES_ONE(pk)
#define CRX_PLANT_READ_TRACK(pk, b) CRX_PLANT_TRACK_ONE(pk, b)
#define CRX_PLANT_NSEG CRX_PLANT_NSEG_ONE
#define CRX_PLANT_ROW(a, i) CRX_PLANT_ROW_ONE(a, i)
#define CRX_PLANT_LAP CRX_PLANT_LAP_ONE
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P

#define CRX_PLANT_KERNEL crx_plant_cars_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams_cars
#define CRX_PLANT_READ_PARAMS(pk, b) CRX_PLANT_PARAMS_CARS(pk, b)
#define CRX_PLANT_P(name) CRX_PLANT_P_CARS(name)
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P
#undef CRX_PLANT_TABLES
#undef CRX_PLANT_READ_TRACK
#undef CRX_PLANT_NSEG
#undef CRX_PLANT_ROW
#undef CRX_PLANT_LAP

#define CRX_PLANT_TABLES(pk) CRX_PLANT_TABLES_SET(pk)
#define CRX_PLANT_READ_TRACK(pk, b) CRX_PLANT_TRACK_SET(pk, b)
#define CRX_PLANT_NSEG CRX_PLANT_NSEG_SET
#define CRX_PLANT_ROW(a, i) CRX_PLANT_ROW_SET(a, i)
#define CRX_PLANT_LAP CRX_PLANT_LAP_SET
#define CRX_PLANT_KERNEL crx_plant_tracks_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams_tracks
#define CRX_PLANT_READ_PARAMS(pk, b) CRX_PLANT_PARAMS_DESC(pk, b)
#define CRX_PLANT_P(name) CRX_PLANT_P_DESC(name)
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P

#define CRX_PLANT_KERNEL crx_plant_tracks_cars_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams_tracks
#define CRX_PLANT_READ_PARAMS(pk, b) CRX_PLANT_PARAMS_CARS(pk, b)
#define CRX_PLANT_P(name) CRX_PLANT_P_CARS(name)
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P
#undef CRX_PLANT_TABLES
#undef CRX_PLANT_READ_TRACK
#undef CRX_PLANT_NSEG
#undef CRX_PLANT_ROW
#undef CRX_PLANT_LAP

hipError_t crx_launch_plant(const crx_plant_kparams& pk, hipStream_t st) { return crx_launch_1d(crx_plant_kernel, pk.batch, 256, 256, st, pk); }
hipError_t crx_launch_plant_cars(const crx_plant_kparams_cars& pk, hipStream_t st) {
    return crx_launch_1d(crx_plant_cars_kernel, pk.batch, 256, 256, st, pk);
}
// pk.params NULL: the descriptor's ten values for every car
hipError_t crx_launch_plant_tracks(const crx_plant_kparams_tracks& pk, hipStream_t st) {
    return crx_launch_1d(pk.params ? crx_plant_tracks_cars_kernel : crx_plant_tracks_kernel, pk.batch, 256, 256, st, pk);
}
