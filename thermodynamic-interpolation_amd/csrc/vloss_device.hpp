// vloss_device.hpp -- the device functions of the velocity loss that more than one kernel unit evaluates and that must agree bit for
// bit wherever they are evaluated: the sigmoid, gamma(t) with its derivative, gamma'(t) alone, and the Philox normal of the z draw.
// Included by vloss_kernels.hip, painn_train_kernels.hip, painn_train_graph_kernels.hip and adw_train_kernels.hip; stated here only.
#pragma once
#include "ti_internal.hpp"
#include "adw_device.hpp"
#include "vloss_normal.hpp"

namespace ti {

constexpr double VL_PI = 3.14159265358979323846;

__device__ __forceinline__ double vl_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// gamma(t) and its derivative (include/ti_hip.h TI_GAMMA_*); VL_SIG_SCALE: the reference holds its 2.2 as a float32 tensor
constexpr double VL_SIG_SCALE = (double)2.2f;
__device__ __forceinline__ void vl_gamma(int kind, double a, double t, double& g, double& gd)
{
    if (kind == TI_GAMMA_BROWNIAN) {
        g = sqrt(a * t * (1.0 - t));
        gd = a * (1.0 - 2.0 * t) / (2.0 * g);
    } else if (kind == TI_GAMMA_SIN2) {
        const double s = sin(VL_PI * t), c = cos(VL_PI * t);
        g = s * s;
        gd = 2.0 * VL_PI * s * c;
    } else {
        const double sp = vl_sigmoid(a * (t - 0.5) + 1.0), sm = vl_sigmoid(a * (t - 0.5) - 1.0);
        g = VL_SIG_SCALE * (sp - sm - vl_sigmoid(1.0 - 0.5 * a) + vl_sigmoid(-1.0 - 0.5 * a));
        gd = VL_SIG_SCALE * a * ((1.0 - sp) * sp - (1.0 - sm) * sm);
    }
}

// gamma'(t) where gamma(t) is not needed (the output gradients of the trainers): the expressions of vl_gamma's gd, written out
__device__ __forceinline__ double vl_gamma_dot(int kind, double a, double t)
{
    if (kind == TI_GAMMA_BROWNIAN) return a * (1.0 - 2.0 * t) / (2.0 * sqrt(a * t * (1.0 - t)));
    if (kind == TI_GAMMA_SIN2) return 2.0 * VL_PI * sin(VL_PI * t) * cos(VL_PI * t);
    const double sp = vl_sigmoid(a * (t - 0.5) + 1.0), sm = vl_sigmoid(a * (t - 0.5) - 1.0);
    return VL_SIG_SCALE * a * ((1.0 - sp) * sp - (1.0 - sm) * sm);
}

// the Philox normal of (seed, trajectory, step, component) exactly as oracle.normal returns it: the counter slots of TI_SCHEME_EM
// (adw_device.hpp ti_normal), Box-Muller by vloss_normal.hpp
__device__ __forceinline__ float vl_normal(uint64_t seed, long long traj, int step, int comp)
{
    uint32_t c[4] = {(uint32_t)traj, (uint32_t)((uint64_t)traj >> 32), (uint32_t)step, (uint32_t)(comp >> 2)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int pair = (comp & 3) >> 1;
    return vl_box_muller(c[2 * pair], c[2 * pair + 1], comp & 1);
}

}  // namespace ti
