// painn_train_graph_body.inc -- the molecule trainer's kernels that read the graph or run over a molecule's entries: the embedding
// inputs, the edge embedding, the message combine forward and reverse, and the output gradient of the loss.  Included once by
// painn_train_kernels.hip (every molecule is the template: pt_*_kernel) and once by painn_train_graph_kernels.hip (molecule b has its
// own live edges, edge types and lv.nat[b] atoms: ptg_*_kernel), so that each pair is one text.  One thread per (row, feature); no
// atomics: a per-node sum walks the template's edges in order.  A dead edge row or a pad node row is kept finite in the forward pass
// and given exactly +0 where it would enter a sum of the reverse pass.
// The including unit defines, and undefines behind the include:
//   TI_TWIN_KERNEL(stem)   the kernel's name
//   TI_TWIN_BLOCK          its block size
//   TI_TWIN_LIVE_PARAM     the trailing parameter `, const PtLive lv`, or nothing
//   TI_PAD_ATOM(a, b)      whether atom a of molecule b is a pad; `false` where there are none
//   TI_PAD_ENTRY(k, b)     whether entry k of molecule b belongs to a pad atom; `false` where there are none
//   TI_BATCH_ATOMS         the atoms of the batch, a double
//   TI_EDGE_TYPES_PARAM    the parameter `const int32_t* __restrict__ etype,` of the template's edge types, or nothing
//   TI_EDGE_TYPE(row)      the type of edge row `row`
//   TI_EDGE_FLAGS(r)       a statement: what TI_EDGE_DEAD reads of molecule r, or nothing
//   TI_EDGE_DEAD(k)        whether template edge k is dead in that molecule; `false` where none is
// In the uniform unit a predicate is `false`, nothing or the plain expression, so a uniform kernel has no instruction of a twin's.

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(embed_in)(float* __restrict__ s_in, const PtEmbedIn e, const PtGraph g TI_TWIN_LIVE_PARAM)
{
    const int K = e.nE * g.F;
    const long long i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= g.R * g.A * K) return;
    const long long n = i / K, r = n / g.A, b = r % e.B;
    const int j = (int)(i - n * K), a = (int)(n - r * g.A), seg = j / g.F, f = j - seg * g.F;
    float v;
    if (seg == 0) v = e.atom_emb[(size_t)e.atom_ids[a] * g.F + f];
    else if (seg < e.nE - 1) {
        float u = (TI_PAD_ATOM(a, b) ? 0.0f : e.cond[(b * g.A + a) * e.ncond + (seg - 1)]) - e.temp_mean;
        u = u / e.temp_range;
        v = pt_posenc(u / e.temp_length, f);
    } else v = pt_posenc(e.t[b] / e.time_length, f);
    s_in[i] = v;
}

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(edge_emb)(float* __restrict__ e0, const float* __restrict__ table, TI_EDGE_TYPES_PARAM
                                                                          const PtGraph g TI_TWIN_LIVE_PARAM)
{
    const long long i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= g.R * g.E * g.F) return;
    const long long row = i / g.F;
    e0[i] = table[(size_t)TI_EDGE_TYPE(row) * g.F + (i - row * g.F)];
}

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(msg_fwd)(float* __restrict__ s_out, float* __restrict__ v_out, const float* __restrict__ s,
                                                                         const float* __restrict__ v, const float* __restrict__ P, const float* __restrict__ Wd,
                                                                         const float* __restrict__ dir, const PtGraph g TI_TWIN_LIVE_PARAM)
{
    const int F = g.F;
    const long long i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= g.R * g.A * F) return;
    const long long n = i / F, r = n / g.A;
    const int f = (int)(i - n * F), a = (int)(n - r * g.A);
    TI_EDGE_FLAGS(r)
    const float vn0 = v[(n * 3) * F + f], vn1 = v[(n * 3 + 1) * F + f], vn2 = v[(n * 3 + 2) * F + f];
    float ds = 0.f, dv0 = 0.f, dv1 = 0.f, dv2 = 0.f;
    for (int k = 0; k < g.E; ++k) {
        if (g.dst[k] != a || TI_EDGE_DEAD(k)) continue;
        const long long row = r * g.E + k, ns = r * g.A + g.src[k], o = row * 5 * F + f;
        const float gates = P[o] * Wd[o], scale = P[o + F] * Wd[o + F], cross = P[o + 4 * F] * Wd[o + 4 * F];
        const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
        const float c0 = d1 * vn2 - d2 * vn1, c1 = d2 * vn0 - d0 * vn2, c2 = d0 * vn1 - d1 * vn0;
        dv0 += scale * d0 + gates * v[(ns * 3) * F + f] + cross * c0;
        dv1 += scale * d1 + gates * v[(ns * 3 + 1) * F + f] + cross * c1;
        dv2 += scale * d2 + gates * v[(ns * 3 + 2) * F + f] + cross * c2;
        ds += P[o + 2 * F] * Wd[o + 2 * F];
    }
    s_out[i] = s[i] + ds;
    v_out[(n * 3) * F + f] = vn0 + dv0; v_out[(n * 3 + 1) * F + f] = vn1 + dv1; v_out[(n * 3 + 2) * F + f] = vn2 + dv2;
}

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(msg_bwd_edge)(float* __restrict__ gP, float* __restrict__ gWd, const float* __restrict__ gs,
                                                                              const float* __restrict__ gv, const float* __restrict__ ge,
                                                                              const float* __restrict__ v, const float* __restrict__ P,
                                                                              const float* __restrict__ Wd, const float* __restrict__ dir,
                                                                              const PtGraph g TI_TWIN_LIVE_PARAM)
{
    const int F = g.F;
    const long long i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= g.R * g.E * F) return;
    const long long row = i / F, r = row / g.E;
    const int f = (int)(i - row * F), k = (int)(row - r * g.E);
    const long long ns = r * g.A + g.src[k], nd = r * g.A + g.dst[k], o = row * 5 * F + f;
    TI_EDGE_FLAGS(r)
    if (TI_EDGE_DEAD(k)) {                                     // +0 into every product and column sum behind it
#pragma unroll
        for (int j = 0; j < 5; ++j) { gP[o + j * F] = 0.0f; gWd[o + j * F] = 0.0f; }
        return;
    }
    const float g0 = gv[(nd * 3) * F + f], g1 = gv[(nd * 3 + 1) * F + f], g2 = gv[(nd * 3 + 2) * F + f];
    const float s0 = v[(ns * 3) * F + f], s1 = v[(ns * 3 + 1) * F + f], s2 = v[(ns * 3 + 2) * F + f];
    const float t0 = v[(nd * 3) * F + f], t1 = v[(nd * 3 + 1) * F + f], t2 = v[(nd * 3 + 2) * F + f];
    const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
    const float c0 = d1 * t2 - d2 * t1, c1 = d2 * t0 - d0 * t2, c2 = d0 * t1 - d1 * t0;
    float gh[5];
    gh[0] = g0 * s0 + g1 * s1 + g2 * s2;                // gates
    gh[1] = g0 * d0 + g1 * d1 + g2 * d2;                // scale
    gh[2] = gs[nd * F + f];                             // ds
    gh[3] = ge ? ge[row * F + f] : 0.0f;                // de
    gh[4] = g0 * c0 + g1 * c1 + g2 * c2;                // cross gates
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        gP[o + j * F] = gh[j] * Wd[o + j * F];
        gWd[o + j * F] = gh[j] * P[o + j * F];
    }
}

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(msg_bwd_node)(float* __restrict__ gs_out, float* __restrict__ gv_out, const float* __restrict__ gs,
                                                                              const float* __restrict__ gv, const float* __restrict__ gin_phi,
                                                                              const float* __restrict__ P, const float* __restrict__ Wd,
                                                                              const float* __restrict__ dir, const PtGraph g TI_TWIN_LIVE_PARAM)
{
    const int F = g.F;
    const long long i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= g.R * g.A * F) return;
    const long long n = i / F, r = n / g.A;
    const int f = (int)(i - n * F), a = (int)(n - r * g.A);
    TI_EDGE_FLAGS(r)
    const float g0 = gv[(n * 3) * F + f], g1 = gv[(n * 3 + 1) * F + f], g2 = gv[(n * 3 + 2) * F + f];
    float as = gs[i], a0 = g0, a1 = g1, a2 = g2;
    for (int k = 0; k < g.E; ++k) {
        if (TI_EDGE_DEAD(k)) continue;
        const long long row = r * g.E + k, o = row * 5 * F + f;
        if (g.src[k] == a) {                                               // an outgoing edge: s[src] of phi's input, gates v[src]
            const long long nd = r * g.A + g.dst[k];
            const float gates = P[o] * Wd[o];
            as += gin_phi[row * 2 * F + f];
            a0 += gates * gv[(nd * 3) * F + f]; a1 += gates * gv[(nd * 3 + 1) * F + f]; a2 += gates * gv[(nd * 3 + 2) * F + f];
        }
        if (g.dst[k] == a) {
            const float cross = P[o + 4 * F] * Wd[o + 4 * F];              // an incoming edge: cross (dir x v[dst]) -> cross (g x dir)
            const float d0 = dir[3 * row], d1 = dir[3 * row + 1], d2 = dir[3 * row + 2];
            a0 += cross * (g1 * d2 - g2 * d1); a1 += cross * (g2 * d0 - g0 * d2); a2 += cross * (g0 * d1 - g1 * d0);
        }
    }
    gs_out[i] = as;
    gv_out[(n * 3) * F + f] = a0; gv_out[(n * 3 + 1) * F + f] = a1; gv_out[(n * 3 + 2) * F + f] = a2;
}

__global__ __launch_bounds__(TI_TWIN_BLOCK) void TI_TWIN_KERNEL(gout)(float* __restrict__ gz, const VlossParams p TI_TWIN_LIVE_PARAM)
{
#pragma clang fp contract(off)
    const long long n = p.B * p.m, i = (long long)blockIdx.x * TI_TWIN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long b = i / p.m;
    if (TI_PAD_ENTRY((int)(i - b * p.m), b)) {
        gz[i] = 0.0f;
        if (p.kind != TI_VLOSS_ONE_SIDED) gz[n + i] = 0.0f;
        return;
    }
    const double d = (double)p.x1[i] - (double)p.x0[i], inv = TI_BATCH_ATOMS;
    if (p.kind == TI_VLOSS_ONE_SIDED) { gz[i] = (float)(((double)p.b[i] - d) / inv); return; }
    const double gzv = vl_gamma_dot(p.gamma, p.a, (double)p.t[b]) * (double)p.z[i];
    gz[i] = (float)(((double)p.b[i] - (d + gzv)) / inv);
    gz[n + i] = (float)(((double)p.b[p.half + i] - (d - gzv)) / inv);
}
