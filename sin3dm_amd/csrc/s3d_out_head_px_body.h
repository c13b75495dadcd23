// s3d_out_head_px_body.h — the ONE source of the pixel-chunk output head's kernels (s3d_kernels.hip includes it once per kernel,
// right behind the kernel's signature; what the block does is described there):
//   k_out_head_px<CQ, FUSED, CARRY, KNOWN>     MULTI = false   the head alone, + p_sample / ddim_sample, + the next in_conv, + the known-region blend
//   k_out_head_px_ms<CQ, CARRY>                MULTI = true    the head + the DPM-Solver++ multistep update
// The including kernel provides: the compile-time constants CQ, FUSED, CARRY, KNOWN, MULTI; OutHeadArgs a; int segs0, segs1;
// s3d_sampler_args sa; InConvCarry cy; KnownArg<KNOWN> kn; MultiArg<MULTI> mu (the last two: empty structs without their flag).
// (A body and not a function template called by the kernels, as s3d_wino24_block.h: as a __device__ __forceinline__ function template
// behind two __global__ wrappers, every one of the fifteen k_out_head_px instantiations came out with other code than it had — up to 7
// more scalar registers, two spilled scalars in five that had none, the known-region ones without CARRY among them, which
// tests/test_edit_resources.py holds to none.  As text they keep their instructions: tools/compare_isa.py s3d_kernels.hip --kernels
// 'k_out_head_px(_ms)?I')
    static_assert(FUSED || !KNOWN, "the blend belongs to the sampler update");
    static_assert(!MULTI || (FUSED && !KNOWN), "the multistep update is a fused step without a known region");
    constexpr int C = 4 * CQ, CPW = C / 4, LANES = 256 / CQ, LD = C + 4;
    __shared__ __attribute__((aligned(16))) float sx[kOhPx * LD];
    __shared__ float sp[4][16][kOhPx];
    __shared__ float sst[64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Hc = a.H + a.D, Wc = a.W + a.D;
    int blk = blockIdx.x, p = 0;
    if (blk >= segs0) { blk -= segs0; p = 1; if (blk >= segs1) { blk -= segs1; p = 2; } }
    // The D x D corner of compose_featmaps (zeros; FUSED: the sampler update with a model output of 0 — a quarter of the composed
    // map at D = H = W) is spread over the pixel blocks: element i = block * 256 + thread (+ k * all threads).  Extra corner
    // blocks behind the pixel blocks were a second, nearly empty round of the chip (768 + 192 blocks on 768 slots: 25 us);
    // here x_t / eps of the thread's first two corner elements are requested with the block's other early loads.
    const long long n_corner = (long long)a.Cout * a.D * a.D;
    const long long corner_stride = 256LL * gridDim.x;
    const long long corner_i0 = (long long)blockIdx.x * 256 + tid;
    constexpr int CU_ = 2;
    size_t corner_o[CU_]; float corner_x[CU_], corner_n[CU_];
    [[maybe_unused]] float corner_p[CU_] = {0.f, 0.f};          // MULTI: x0_prev there
#pragma unroll
    for (int u = 0; u < CU_; ++u) {
        const long long i = corner_i0 + u * corner_stride;
        corner_o[u] = 0; corner_x[u] = corner_n[u] = 0.f;
        if (i < n_corner) {
            const int dx = int(i % a.D), dy = int((i / a.D) % a.D), co = int(i / a.D / a.D);
            corner_o[u] = ((size_t(b) * a.Cout + co) * Hc + a.H + dy) * Wc + a.W + dx;
            // (CARRY: requested behind the output loop instead — their latency then runs under the in_conv tail; kept from here they
            // were live across the whole kernel and spilled behind a vmcnt(0) at its very start)
            if (FUSED && !CARRY) { corner_x[u] = sa.x[corner_o[u]]; if (sa.noise) corner_n[u] = sa.noise[corner_o[u]]; }
        }
    }
    const int h = a.h[p], w = a.wd[p];
    const int len = p == 2 ? h : w, nseg = (len + kOhPx - 1) / kOhPx;
    const int line = blk / nseg, s0 = (blk % nseg) * kOhPx;
    // the plane's weight rows [Cout][C] are requested NOW and parked in registers: read from memory inside the contraction
    // (wave-uniform addresses, eight 16-byte loads and a full wait per pair of output channels) they were ~8 us of exposed L2
    // round trips per block (batch 8: 171 -> see profiles/r04_out_head.txt); they move into the staging area once every lane
    // holds its activations
    constexpr int kWIts = (16 * CQ + 255) / 256;             // float4 items of Cout <= 16 rows per thread
    float4 wreg[kWIts];
#pragma unroll
    for (int k = 0; k < kWIts; ++k) {
        const int it = tid + 256 * k;
        wreg[k] = it < a.Cout * CQ ? reinterpret_cast<const float4*>(a.w + size_t(p) * a.Cout * C)[it] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // FUSED: x_t and the step's eps of this thread's output positions are requested NOW — as the tail of the block (behind the
    // last barrier) their latency was the block's critical path: 31 us per launch instead of 15 + 7 for head + sampler kernel
    constexpr int kOutIts = 16 * kOhPx / 256;                 // Cout <= 16
    float pre_x[kOutIts], pre_n[kOutIts];
    [[maybe_unused]] float pre_p[kOutIts];                    // MULTI: x0_prev of the output positions
    [[maybe_unused]] SamplerCoef sc;
    [[maybe_unused]] MultistepCoef mcf;
    if (FUSED) {
#pragma unroll
        for (int k = 0; k < kOutIts; ++k) {
            const int it = tid + 256 * k, co = it >> 6, e = it & 63;
            pre_x[k] = pre_n[k] = 0.f;
            if constexpr (MULTI) pre_p[k] = 0.f;
            if (co < a.Cout && s0 + e < len) {
                const int sy = p == 2 ? a.H + line : line, sx0 = p == 1 ? a.W + s0 : s0;
                const size_t o = ((size_t(b) * a.Cout + co) * Hc + sy) * Wc + sx0 + e;
                pre_x[k] = sa.x[o];
                if (sa.noise) pre_n[k] = sa.noise[o];
            }
        }
        if constexpr (MULTI) mcf = multistep_coef(sa, mu.ms, int(sa.t[b]));
        else sc = sampler_coef(sa, int(sa.t[b]));             // (t, then the seven table entries it selects: two dependent round trips, behind the requests above)
    }
    KnownCoef kc{0.f, 0.f};
    if constexpr (KNOWN) kc = known_coef(kn.kr, sa.T, int(sa.t[b]));
    const float* st = sst;
    if (a.mr) {
        if (tid < 32) {
            const float* mr = a.mr + ((size_t(b) * 3 + p) * 32 + tid) * 2;
            sst[tid] = mr[0]; sst[32 + tid] = mr[1];
        }
    } else {
        // the statistics of the head's input from its producer's partial sums, as k_gn_act does it: one k_gn_finalize launch less
        // on the step's dependent chain (the L2-hot reads run beside the x_t / eps requests above)
        st = gn_stats_from_parts(a.ps, b, p, reinterpret_cast<double*>(sx), nullptr);
    }
    __syncthreads();
    {
        const int q = tid % CQ, l = tid / CQ;
        constexpr int cg = C / 32;
        float A[4], Bc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * q + k, g = c / cg;
            A[k] = st[32 + g] * a.gamma[p][c];
            Bc[k] = a.beta[p][c] - A[k] * st[g];
        }
        if (!a.mr) __syncthreads();                         // the added statistics live in sx, which the staging below overwrites
        const float* xb = a.x[p] + size_t(b) * h * w * C;
#pragma unroll
        for (int k = 0; k < kOhPx / LANES; ++k) {
            const int e = k * LANES + l;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s0 + e < len) {
                const int y = p == 2 ? s0 + e : line, xx = p == 2 ? line : s0 + e;
                const float4 v = reinterpret_cast<const float4*>(xb + (size_t(y) * w + xx) * C)[q];
                o.x = silu_f(fmaf(v.x, A[0], Bc[0])); o.y = silu_f(fmaf(v.y, A[1], Bc[1]));
                o.z = silu_f(fmaf(v.z, A[2], Bc[2])); o.w = silu_f(fmaf(v.w, A[3], Bc[3]));
            }
            *reinterpret_cast<float4*>(sx + e * LD + 4 * q) = o;
        }
    }
    __syncthreads();
    {
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), e = tid & 63;
        float act[CPW];
#pragma unroll
        for (int j = 0; j < CPW / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(sx + e * LD + wv * CPW + 4 * j);
            act[4 * j] = v.x; act[4 * j + 1] = v.y; act[4 * j + 2] = v.z; act[4 * j + 3] = v.w;
        }
        __syncthreads();                                    // every lane holds its activations: the staging area takes the weight rows
#pragma unroll
        for (int k = 0; k < kWIts; ++k) {
            const int it = tid + 256 * k;
            if (it < 16 * CQ) reinterpret_cast<float4*>(sx)[it] = wreg[k];
        }
        __syncthreads();
        const float* wb = sx + wv * CPW;                    // [Cout][C]; wave-uniform addresses: LDS broadcast reads
        for (int co = 0; co < a.Cout; ++co) {
            const float4* wr = reinterpret_cast<const float4*>(wb + co * C);
            float s0a = 0.f, s1a = 0.f;
#pragma unroll
            for (int j = 0; j < CPW / 4; ++j) {
                const float4 w4 = wr[j];
                s0a = fmaf(act[4 * j], w4.x, s0a); s1a = fmaf(act[4 * j + 1], w4.y, s1a);
                s0a = fmaf(act[4 * j + 2], w4.z, s0a); s1a = fmaf(act[4 * j + 3], w4.w, s1a);
            }
            sp[wv][co][e] = s0a + s1a;
        }
    }
    // MULTI: x0_prev of this thread's output positions and of its two pre-fetched corner elements is requested HERE, behind the
    // contraction, not with x_t and eps at the top (the barrier and the LDS reads of the output loop run over the latency, and the other
    // blocks of the CU over the rest).  Held across the contraction, four more registers were live at the kernel's widest point: the
    // CQ = 32 CARRY form spilled two behind its 168, the CQ = 64 forms took four more than their default counterparts — y0 / mask /
    // eps_known of the KNOWN form are read late for the same reason.
    if constexpr (MULTI) {
        if (mu.ms.order == 2) {
#pragma unroll
            for (int k = 0; k < kOutIts; ++k) {
                const int it = tid + 256 * k, co = it >> 6, e = it & 63;
                if (co < a.Cout && s0 + e < len) {
                    const int sy = p == 2 ? a.H + line : line, sx0 = p == 1 ? a.W + s0 : s0;
                    pre_p[k] = mu.ms.x0_prev[((size_t(b) * a.Cout + co) * Hc + sy) * Wc + sx0 + e];
                }
            }
            if constexpr (!CARRY) {
#pragma unroll
                for (int u = 0; u < CU_; ++u)
                    if (corner_i0 + u * corner_stride < n_corner) corner_p[u] = mu.ms.x0_prev[corner_o[u]];
            }
        }
    }
    __syncthreads();
    float xnext[kOutIts];
#pragma unroll
    for (int k = 0; k < kOutIts; ++k) xnext[k] = 0.f;
    // CARRY: the next in_conv's weight rows for input channels 0..7 are requested now (their latency runs under the output loop), the
    // other eight once the x_{t-1} values are staged
    float4 wA[8], wB[8];
    float4 biasn = make_float4(0, 0, 0, 0);
    if (FUSED && CARRY) {
        const float4* wq0 = reinterpret_cast<const float4*>(cy.wT + size_t(p) * cy.Cin * C) + tid % CQ;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) wA[ci] = ci < cy.Cin ? wq0[size_t(ci) * CQ] : make_float4(0, 0, 0, 0);
        biasn = reinterpret_cast<const float4*>(cy.bias + size_t(p) * C)[tid % CQ];
    }
#pragma unroll
    for (int k = 0; k < kOutIts; ++k) {
        const int it = tid + 256 * k, co = it >> 6, e = it & 63;
        if (co >= a.Cout || s0 + e >= len) continue;
        const float v = ((sp[0][co][e] + sp[1][co][e]) + (sp[2][co][e] + sp[3][co][e])) + a.bias[p * a.Cout + co];
        const int sy = p == 2 ? a.H + line : line, sx0 = p == 1 ? a.W + s0 : s0;
        const size_t o = ((size_t(b) * a.Cout + co) * Hc + sy) * Wc + sx0 + e;
        if (!FUSED || (!KNOWN && !MULTI && a.out)) a.out[o] = v;
        if (FUSED) {
            float xprev;
            if constexpr (KNOWN) xprev = sampler_element_known<true>(sa, sc, kn.kr, kc, (long long)o, v, pre_x[k], pre_n[k]);
            else if constexpr (MULTI) xprev = multistep_element(sa, mu.ms, mcf, (long long)o, v, pre_x[k], pre_n[k], pre_p[k]);
            else xprev = sampler_element(sa, sc, (long long)o, v, pre_x[k], pre_n[k]);
            if (CARRY) xnext[k] = xprev;
        }
    }
    if (FUSED && CARRY) {
#pragma unroll
        for (int u = 0; u < CU_; ++u) {
            const long long i = (long long)blockIdx.x * 256 + tid + u * corner_stride;
            if (i < n_corner) {
                const int dx = int(i % a.D), dy = int((i / a.D) % a.D), co = int(i / a.D / a.D);
                corner_o[u] = ((size_t(b) * a.Cout + co) * Hc + a.H + dy) * Wc + a.W + dx;
                corner_x[u] = sa.x[corner_o[u]]; if (sa.noise) corner_n[u] = sa.noise[corner_o[u]];
                if constexpr (MULTI) { if (mu.ms.order == 2) corner_p[u] = mu.ms.x0_prev[corner_o[u]]; }
            }
        }
        // ---- the next step's in_conv on this block's x_{t-1} (k_in_conv_lds<32, CQ>, twice).  sx is dead since the barrier above.
        constexpr int LANES_I = 256 / CQ, PXI = 32;
        float (*sxn)[16] = reinterpret_cast<float (*)[16]>(sx);                        // [64 pixels][16 input channels]
        float (*sred)[LANES_I][C] = reinterpret_cast<float (*)[LANES_I][C]>(sx + kOhPx * 16);      // [sum | sumsq][pixel lane][channel]
        static_assert(kOhPx * 16 + 2 * LANES_I * C <= kOhPx * LD, "carry scratch inside the staging area");
#pragma unroll
        for (int k = 0; k < kOutIts; ++k) {
            const int it = tid + 256 * k, co = it >> 6, e = it & 63;
            sxn[e][co] = (co < cy.Cin && s0 + e < len) ? xnext[k] : 0.f;               // (channels Cin..15 and pixels past the line: zeros, as k_in_conv_lds stages them)
        }
        const int q = tid % CQ, lp = tid / CQ;
        const float4* wq = reinterpret_cast<const float4*>(cy.wT + size_t(p) * cy.Cin * C) + q;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) wB[ci] = 8 + ci < cy.Cin ? wq[size_t(8 + ci) * CQ] : make_float4(0, 0, 0, 0);
        const int nseg_in = (len + PXI - 1) / PXI;
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < kOhPx / PXI; ++hh) {
            const int s0i = s0 + hh * PXI;
            if (s0i >= len) break;                                                     // (block-uniform: no such in_conv block)
            // every output's chain is bias, then input channels 0..15 in order (k_in_conv_lds's)
            constexpr int NK = PXI / LANES_I;
            float4 acc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k] = biasn;
#pragma unroll
            for (int half8 = 0; half8 < 2; ++half8) {
                const float4* wvn = half8 ? wB : wA;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int e = k * LANES_I + lp;
#pragma unroll
                    for (int c4 = 0; c4 < 2; ++c4) {
                        const float4 v = *reinterpret_cast<const float4*>(&sxn[hh * PXI + e][(half8 * 2 + c4) * 4]);
                        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float4 ww = wvn[c4 * 4 + j];
                            acc[k].x = fmaf(vv[j], ww.x, acc[k].x); acc[k].y = fmaf(vv[j], ww.y, acc[k].y);
                            acc[k].z = fmaf(vv[j], ww.z, acc[k].z); acc[k].w = fmaf(vv[j], ww.w, acc[k].w);
                        }
                    }
                }
            }
            float gs[4] = {0.f, 0.f, 0.f, 0.f}, gss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int e = k * LANES_I + lp;
                if (s0i + e >= len) continue;
                const int y = p == 2 ? s0i + e : line, xx = p == 2 ? line : s0i + e;
                reinterpret_cast<float4*>(cy.out[p] + ((size_t(b) * h + y) * w + xx) * C)[q] = acc[k];
                gs[0] += acc[k].x; gs[1] += acc[k].y; gs[2] += acc[k].z; gs[3] += acc[k].w;
                gss[0] = fmaf(acc[k].x, acc[k].x, gss[0]); gss[1] = fmaf(acc[k].y, acc[k].y, gss[1]); gss[2] = fmaf(acc[k].z, acc[k].z, gss[2]); gss[3] = fmaf(acc[k].w, acc[k].w, gss[3]);
            }
            if (cy.part) {
                if (hh) __syncthreads();                                               // the previous half's partial sums have been read
#pragma unroll
                for (int k = 0; k < 4; ++k) { sred[0][lp][4 * q + k] = gs[k]; sred[1][lp][4 * q + k] = gss[k]; }
                __syncthreads();
                if (tid < 32) {
                    constexpr int cg = C / 32;
                    const int g = tid;
                    double S = 0, SS = 0;
                    for (int l = 0; l < LANES_I; ++l)
#pragma unroll
                        for (int k = 0; k < cg; ++k) { S += sred[0][l][cg * g + k]; SS += sred[1][l][cg * g + k]; }
                    const int blk_in = line * nseg_in + s0i / PXI;
                    double* o = cy.part + (((size_t(b) * 3 + p) * 32 + g) * cy.maxparts + blk_in) * 2;
                    o[0] = S; o[1] = SS;
                }
            }
        }
    }
    // (the corner index again from an opaque thread id: kept from the top of the kernel it was a 64-bit value live across the CARRY tail — spilled)
    int tid_c = threadIdx.x;
    if (CARRY) asm volatile("" : "+v"(tid_c));
    const long long corner_i1 = CARRY ? (long long)blockIdx.x * 256 + tid_c : corner_i0;
#pragma unroll
    for (int u = 0; u < CU_; ++u) {
        if (corner_i1 + u * corner_stride >= n_corner) continue;
        if (!FUSED || (!KNOWN && !MULTI && a.out)) a.out[corner_o[u]] = 0.f;
        if constexpr (KNOWN) sampler_element_known<true>(sa, sc, kn.kr, kc, (long long)corner_o[u], 0.f, corner_x[u], corner_n[u]);
        else if constexpr (MULTI) multistep_element(sa, mu.ms, mcf, (long long)corner_o[u], 0.f, corner_x[u], corner_n[u], corner_p[u]);
        else if (FUSED) sampler_element(sa, sc, (long long)corner_o[u], 0.f, corner_x[u], corner_n[u]);
    }
    for (long long i = corner_i1 + CU_ * corner_stride; i < n_corner; i += corner_stride) {      // (shapes with D*D > 2 x the plane pixels)
        const int dx = int(i % a.D), dy = int((i / a.D) % a.D), co = int(i / a.D / a.D);
        const size_t o = ((size_t(b) * a.Cout + co) * Hc + a.H + dy) * Wc + a.W + dx;
        if (!FUSED || (!KNOWN && !MULTI && a.out)) a.out[o] = 0.f;
        if constexpr (KNOWN) sampler_element_known<true>(sa, sc, kn.kr, kc, (long long)o, 0.f);
        else if constexpr (MULTI) multistep_element(sa, mu.ms, mcf, (long long)o, 0.f);
        else if (FUSED) sampler_element(sa, sc, (long long)o, 0.f);
    }
