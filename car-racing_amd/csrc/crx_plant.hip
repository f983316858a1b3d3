// crx_plant.hip -- the plant, the two inclusions of crx_plant_step.h:
//   crx_plant_kernel        one control step of the plant for a batch of vehicles, one BicycleDynamicsParam set for the launch
//   crx_plant_cars_kernel   the same step with one BicycleDynamicsParam set per vehicle (params[batch][10])
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
#define CRX_PLANT_KERNEL crx_plant_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams
#define CRX_PLANT_READ_PARAMS(pk, b)
#define CRX_PLANT_P(name) d.name
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P

#define CRX_PLANT_KERNEL crx_plant_cars_kernel
#define CRX_PLANT_KPARAMS crx_plant_kparams_cars
#define CRX_PLANT_READ_PARAMS(pk, b)                                                                                                  \
    const double* row = pk.params + CRX_PLANT_NPARAM * (size_t)b;                                                                     \
    const double car_m = row[0], car_lf = row[1], car_lr = row[2], car_Iz = row[3], car_Df = row[4], car_Cf = row[5], car_Bf = row[6], \
                 car_Dr = row[7], car_Cr = row[8], car_Br = row[9];
#define CRX_PLANT_P(name) car_##name
#include "crx_plant_step.h"
#undef CRX_PLANT_KERNEL
#undef CRX_PLANT_KPARAMS
#undef CRX_PLANT_READ_PARAMS
#undef CRX_PLANT_P

hipError_t crx_launch_plant(const crx_plant_kparams& pk, hipStream_t st) { return crx_launch_1d(crx_plant_kernel, pk.batch, 256, 256, st, pk); }
hipError_t crx_launch_plant_cars(const crx_plant_kparams_cars& pk, hipStream_t st) {
    return crx_launch_1d(crx_plant_cars_kernel, pk.batch, 256, 256, st, pk);
}
