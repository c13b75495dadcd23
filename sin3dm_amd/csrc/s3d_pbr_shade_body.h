// s3d_pbr_shade_body.h — the ONE source of the PBR shade-and-resolve kernels (included right behind the kernel's signature, as
// s3d_out_head_px_body.h is): thread = pixel, its ss x ss samples in row order, as k_render_shade.
//   k_render_shade_pbr      (s3d_render_pbr.hip)   LIT = false   every light reaches every sample
//   k_render_shade_pbr_lit  (s3d_ray.hip)          LIT = true    light k is skipped where bit k of the sample's mask byte is clear
// The including kernel provides: PbrArgs a; the compile-time constant LIT; const unsigned char* lit ([hs][ws], read only when LIT).
// As text, k_render_shade_pbr keeps the instructions it had before the mask existed (tests/test_render_pbr_resources.py holds its
// registers to the table of DESIGN.md §24).
    const ShadeArgs& s = a.s;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)s.W * s.H) return;
    const int ix = int(p % s.W), iy = int(p / s.W);
    const float kPi = 3.14159265358979323846f;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int covered = 0;
    for (int j = 0; j < s.ss; ++j)
        for (int i = 0; i < s.ss; ++i) {
            const int sx = ix * s.ss + i, sy = iy * s.ss + j;
            const int f = s.face_id[(long long)sy * s.ws + sx];
            ScreenTri t;
            if (f < 0 || f >= s.F || load_screen_tri(s.xy, s.inv_w, s.V, s.faces, f, t) != TRI_OK) continue;
            float b0, b1, b2;
            sample_barycentrics(t, sx, sy, b0, b1, b2);
            // ---- the shading normal: flat, towards the camera by the integer rule
            float N[3];
            bool front;
            face_normal(s.verts, t, s.front_sign, N, front);
            const bool has_flat = normalize3(N);
            if (!has_flat) { N[0] = 0.0f; N[1] = 0.0f; N[2] = 0.0f; }
            if (!front) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
            if (a.normals && has_flat) {                       // smooth: the mix of the corners' normals, unless it is unusable
                const float* n0 = a.normals + t.v0 * 3LL;
                const float* n1 = a.normals + t.v1 * 3LL;
                const float* n2 = a.normals + t.v2 * 3LL;
                const bool any_zero = (n0[0] == 0.0f && n0[1] == 0.0f && n0[2] == 0.0f) || (n1[0] == 0.0f && n1[1] == 0.0f && n1[2] == 0.0f) ||
                                      (n2[0] == 0.0f && n2[1] == 0.0f && n2[2] == 0.0f);
                float mix[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) mix[k] = b0 * n0[k] + b1 * n1[k] + b2 * n2[k];
                if (!any_zero && normalize3(mix)) {
                    if (!front) { mix[0] = -mix[0]; mix[1] = -mix[1]; mix[2] = -mix[2]; }
                    if (dot3(mix, N) > 0.0f) { N[0] = mix[0]; N[1] = mix[1]; N[2] = mix[2]; }
                }
            }
            // ---- the material
            float albedo[3] = {1.0f, 1.0f, 1.0f}, metal = 0.0f, rough = 0.5f;
            float tu = 0.0f, tv = 0.0f;
            int m = -1;
            if (a.pbr) {
                m = s.face_mat ? s.face_mat[f] : 0;
                if (m < 0 || m >= s.M) m = -1;
                if (s.uv) sample_uv(s.uv, f, t.swapped, b0, b1, b2, tu, tv);
                if (m >= 0) {
                    albedo[0] = a.fac[m][0]; albedo[1] = a.fac[m][1]; albedo[2] = a.fac[m][2];
                    metal = a.fac[m][3]; rough = a.fac[m][4];
                    if (s.uv) {
                        if (a.tab[m][0][1] > 0) tex_bilinear<3>(s.img, a.tab[m][0][0], int(a.tab[m][0][1]), int(a.tab[m][0][2]), tu, tv, albedo);
                        if (a.tab[m][1][1] > 0) tex_bilinear<1>(s.img, a.tab[m][1][0], int(a.tab[m][1][1]), int(a.tab[m][1][2]), tu, tv, &metal);
                        if (a.tab[m][2][1] > 0) tex_bilinear<1>(s.img, a.tab[m][2][0], int(a.tab[m][2][1]), int(a.tab[m][2][2]), tu, tv, &rough);
                    }
                }
            } else {
                base_colour(s, t, f, b0, b1, b2, albedo);
            }
            // ---- the normal map, in the face's tangent frame made orthonormal around N
            if (a.pbr && m >= 0 && a.pass != S3D_RENDER_PASS_GEO && a.tangents && s.uv && has_flat && a.tab[m][3][1] > 0) {
                const float* tg = a.tangents + (long long)f * 6;
                float T[3] = {tg[0], tg[1], tg[2]};
                const float B[3] = {tg[3], tg[4], tg[5]};
                const float nt = dot3(N, T);
#pragma unroll
                for (int k = 0; k < 3; ++k) T[k] = T[k] - N[k] * nt;
                if (normalize3(T)) {
                    float Bp[3], tx[3];
                    cross3(N, T, Bp);
                    const float sg = dot3(Bp, B) < 0.0f ? -1.0f : 1.0f;
                    tex_bilinear<3>(s.img, a.tab[m][3][0], int(a.tab[m][3][1]), int(a.tab[m][3][2]), tu, tv, tx);
#pragma unroll
                    for (int k = 0; k < 3; ++k) tx[k] = 2.0f * tx[k] - 1.0f;
                    float Nm[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) Nm[k] = tx[0] * T[k] + tx[1] * (sg * Bp[k]) + tx[2] * N[k];
                    if (normalize3(Nm)) { N[0] = Nm[0]; N[1] = Nm[1]; N[2] = Nm[2]; }
                }
            }
            if (a.pass == S3D_RENDER_PASS_GEO) {
                albedo[0] = albedo[1] = albedo[2] = S3D_RENDER_GEO_GREY;
                metal = 0.0f; rough = 0.5f;
            }
            // ---- the value of the pass
            float out[3];
            if (a.pass == S3D_RENDER_PASS_ALBEDO) {
                out[0] = albedo[0]; out[1] = albedo[1]; out[2] = albedo[2];
            } else if (a.pass == S3D_RENDER_PASS_METALLIC) {
                out[0] = out[1] = out[2] = metal;
            } else if (a.pass == S3D_RENDER_PASS_ROUGHNESS) {
                out[0] = out[1] = out[2] = rough;
            } else if (a.pass == S3D_RENDER_PASS_NORMAL) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = 0.5f * N[k] + 0.5f;
            } else {
                const float r = fminf(fmaxf(rough, S3D_RENDER_MIN_ROUGHNESS), 1.0f);
                const float alpha = r * r, a2 = alpha * alpha, kk = 0.5f * alpha;
                // the point on the face, and the unit vector from it to the eye
                const float* P0 = s.verts + t.v0 * 3LL;
                const float* P1 = s.verts + t.v1 * 3LL;
                const float* P2 = s.verts + t.v2 * 3LL;
                float Vv[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) Vv[k] = a.eye[k] - (b0 * P0[k] + b1 * P1[k] + b2 * P2[k]);
                if (!normalize3(Vv)) { Vv[0] = N[0]; Vv[1] = N[1]; Vv[2] = N[2]; }
                const float NV = fmaxf(dot3(N, Vv), 1e-4f);
                const float gv = __fdiv_rn(NV, NV * (1.0f - kk) + kk);
                float F0[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    F0[k] = 0.04f * (1.0f - metal) + albedo[k] * metal;
                    out[k] = a.ambient * albedo[k];
                }
#pragma unroll 1
                for (int li = 0; li < a.n_lights; ++li) {       // (rolled: the lights stay in the argument block, not in registers)
                    if constexpr (LIT) {                        // the shadow mask: a light that does not reach the sample adds nothing
                        if (!((lit[(long long)sy * s.ws + sx] >> li) & 1)) continue;
                    }
                    if (li < kMaxLights) {
                        const float L[3] = {a.lights[li][0], a.lights[li][1], a.lights[li][2]};
                        const float NL = fmaxf(dot3(N, L), 0.0f);
                        float Hh[3] = {L[0] + Vv[0], L[1] + Vv[1], L[2] + Vv[2]};
                        if (!normalize3(Hh)) { Hh[0] = N[0]; Hh[1] = N[1]; Hh[2] = N[2]; }
                        const float NH = dot3(N, Hh), VH = fminf(fmaxf(dot3(Vv, Hh), 0.0f), 1.0f);
                        const float x = 1.0f - VH, x2 = x * x, x5 = x2 * x2 * x;
                        const float dd = NH * NH * (a2 - 1.0f) + 1.0f;
                        const float D = __fdiv_rn(a2, kPi * dd * dd);
                        const float G = __fdiv_rn(NL, NL * (1.0f - kk) + kk) * gv;
                        const float spec = __fdiv_rn(kPi * D * G, 4.0f * NL * NV + 1e-6f);
                        const float w = a.lights[li][3] * NL;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float Fk = F0[k] + (1.0f - F0[k]) * x5;
                            out[k] += w * ((1.0f - Fk) * (1.0f - metal) * albedo[k] + spec * Fk);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += fminf(fmaxf(out[k], 0.0f), 1.0f);
            ++covered;
        }
    unsigned char o[4] = {0, 0, 0, 0};
    if (covered) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (unsigned char)int(__fdiv_rn(acc[k], float(covered)) * 255.0f + 0.5f);
        o[3] = (unsigned char)int(__fdiv_rn(float(covered), float(s.ss * s.ss)) * 255.0f + 0.5f);
    }
    s.rgba[p * 4] = o[0]; s.rgba[p * 4 + 1] = o[1]; s.rgba[p * 4 + 2] = o[2]; s.rgba[p * 4 + 3] = o[3];
