// vloss_state_body.inc -- the velocity loss's kernels over a molecule's entries: the interpolant's states, their centring and the
// per-molecule reduction.  Included once by vloss_kernels.hip (every molecule has p.A atoms: vloss_*_kernel) and once by
// painn_train_graph_kernels.hip (molecule b has lv.nat[b] atoms and pads behind them: ptg_*_kernel), so that each pair is one text.
// The including unit defines, and undefines behind the include:
//   TI_TWIN_KERNEL(stem)   the kernel's name
//   TI_TWIN_BLOCK          its block size
//   TI_TWIN_LIVE_PARAM     the trailing parameter `, const PtLive lv`, or nothing
//   TI_MOL_ATOMS(b)        the atoms of molecule b
//   TI_MOL_ENTRIES(b)      the entries of molecule b: its atoms times p.m / p.A
//   TI_PAD_ENTRY(k, b)     whether entry k of molecule b belongs to a pad atom; `false` where there are none
//   TI_BATCH_ATOMS         the atoms of the batch, a double
// In the uniform unit a predicate is `false`, nothing or the plain expression, so a uniform kernel has no instruction of a twin's.

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(interp)(VlossParams p TI_TWIN_LIVE_PARAM)
{
    const long long n = p.B * p.m, i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long b = i / p.m;
    const int comp = (int)(i - b * p.m);
    const bool two = p.kind != TI_VLOSS_ONE_SIDED;
    if (TI_PAD_ENTRY(comp, b)) {                                        // nothing is read, nothing is drawn
        if (two) p.z[i] = 0.0f;
        if (p.center != TI_CENTER_NONE) { p.raw[i] = 0.0; if (two) p.raw[n + i] = 0.0; }
        return;
    }
    const double t = (double)p.t[b], x0 = (double)p.x0[i], x1 = (double)p.x1[i];
    double xp, xm = 0.0;
    if (p.kind == TI_VLOSS_ONE_SIDED) xp = t * x1 + (1.0 - t) * x0;
    else {
        const float z = p.z_in ? p.z_in[i] : vl_normal(p.seed, p.traj0 + b, p.draw, comp);
        p.z[i] = z;
        double g, gd;
        vl_gamma(p.gamma, p.a, t, g, gd);
        const double it = (1.0 - t) * x0 + t * x1, gz = g * (double)z;
        xp = it + gz; xm = it - gz;
    }
    if (p.center == TI_CENTER_NONE) { p.xt[i] = (float)xp; if (two) p.xt[p.half + i] = (float)xm; }
    else { p.raw[i] = xp; if (two) p.raw[n + i] = xm; }
}

// blockIdx.y: the half (plus, minus)
__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(center)(VlossParams p TI_TWIN_LIVE_PARAM)
{
    const long long n = p.B * p.m, i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int half = blockIdx.y, nc = p.m / p.A;
    const long long b = i / p.m;
    const int nb = TI_MOL_ATOMS(b);
    if (TI_PAD_ENTRY((int)(i - b * p.m), b)) return;                    // launch_ptg_pad writes it
    const int c = (int)(i - b * p.m) % nc;
    const double* raw = p.raw + (size_t)half * n;
    double mean;
    if (p.center == TI_CENTER_BATCH) mean = p.colsum[half * nc + c] / TI_BATCH_ATOMS;
    else {
        double s = 0.0;
        for (int a = 0; a < nb; ++a) s += raw[b * p.m + a * nc + c];
        mean = s / (double)nb;
    }
    p.xt[(size_t)half * p.half + i] = (float)(raw[i] - mean);
}

// one thread per molecule / row, its entries in order.  Contraction off: every product and sum below is rounded on its own, so l_b is
// the IEEE evaluation of the header's expression, operation by operation.  A fused d + gamma' z is the more exact one, but where d and
// gamma' z cancel it differs from the plain evaluation by far more than the roundings of the terms, and which products fuse would be
// the compiler's choice.
__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(reduce)(VlossParams p TI_TWIN_LIVE_PARAM)
{
#pragma clang fp contract(off)
    const long long b = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (b >= p.B) return;
    const long long o = b * p.m;
    const int m = TI_MOL_ENTRIES(b);
    const bool two = p.kind != TI_VLOSS_ONE_SIDED;
    double g = 0.0, gd = 0.0;
    if (two) vl_gamma(p.gamma, p.a, (double)p.t[b], g, gd);
    double acc = 0.0;
    for (int k = 0; k < m; ++k) {
        const double d = (double)p.x1[o + k] - (double)p.x0[o + k], bp = (double)p.b[o + k];
        acc += 0.5 * bp * bp;
        if (two) {
            const double gz = gd * (double)p.z[o + k], bm = (double)p.b[p.half + o + k];
            acc -= (d + gz) * bp;
            acc += 0.5 * bm * bm;
            acc -= (d - gz) * bm;
        } else acc -= d * bp;
    }
    p.loss[b] = acc;
}
