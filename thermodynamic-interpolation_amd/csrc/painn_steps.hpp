// painn_steps.hpp -- private header of the molecule trainer's many-step call (include/ti_hip.h ti_painn_train_steps,
// ti_painn_train_best, ti_painn_train_noise): the launchers of painn_steps_kernels.hip (gather of a minibatch with its conditioning,
// the forward-only log entry, the best-weights rule) and of painn_noise_kernels.hip (the latent base samples).  Shared by those two
// units and api_painn_train.hip only.
#pragma once
#include "painn_train.hpp"

namespace ti {

// The minibatch of a step from the resident sets: gx0, gx1 [B][A][3] = rows idx0[b] of x0 [n0][A][3] and idx1[b] of x1 [n1][A][3]
// (idx == NULL: row b; x0 == NULL: gx0 is not written), cond [B][A][ncond] = (temp0[idx0[b]], temp1[idx1[b]]) (ncond == 2),
// temp1[idx1[b]] (ncond == 1) or nothing.  An index outside its set reads row 0 (the host has refused it before).
struct PtGather {
    float *gx0, *gx1, *cond;
    const float *x0, *x1, *temp0, *temp1;
    const long long *idx0, *idx1;
    long long n0, n1, B;
    int A, ncond;
};
hipError_t launch_ptsteps_gather(const PtGather& g, hipStream_t st);

// log[0] = loss_sum[0] / divisor: the mean loss of a forward-only step, non-finite values as they are
hipError_t launch_ptsteps_log(double* log, const double* loss_sum, double divisor, hipStream_t st);

// The best-weights rule of a step, between its passes and its update.  The step's loss is loss_sum / divisor where both batch-wide
// sums are finite (the optimiser's own test: a step it skips never wins).  Where that loss is strictly below best[0], keep copies
// w [n] into best_w; commit, launched behind it, then sets best = (loss, step).  best [2]: the loss and the step as doubles.
struct PtBest {
    double* best_w; const double* w; size_t n;
    double* best; const double *loss_sum, *sumsq; double divisor, step;
};
hipError_t launch_ptsteps_best_keep(const PtBest& b, hipStream_t st);
hipError_t launch_ptsteps_best_commit(const PtBest& b, hipStream_t st);

// The latent base samples of B molecules (include/ti_hip.h ti_painn_train_noise): xc [B][A][3] fp64 scratch for the centred draws,
// x1 [B][A][3] (read where aligned), out_x0 [B][A][3], out_rot [B][3][3] or NULL.  One thread per molecule.
struct PtNoise {
    uint64_t seed; long long traj0; int draw;
    const float* x1; long long B; int A; int aligned;
    double* xc; float* out_x0; double* out_rot;
};
hipError_t launch_ptnoise(const PtNoise& p, hipStream_t st);

}  // namespace ti
