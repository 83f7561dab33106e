/* CPU restatement (plain C + OpenMP, fp32) of the selective scan and causal conv1d the reference reaches through
 * mamba_ssm.Mamba.forward (/root/reference/caduceus/modeling_caduceus.py:11,128,130; algorithm of the un-vendored
 * dependencies mamba-ssm==1.2.0.post1 `selective_scan_ref` and causal-conv1d==1.2.0.post2, restated from their
 * published definition -- SURVEY.md section 7.2).
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE: used by tests/ as a second, independent checker at sizes where the
 * torch loop in oracle_model.py is too slow, and by bench.py's `cpu_baseline` leg ("port", all host cores).
 * Pinned by tests/test_oracle_golden.py against the committed third-party vectors (tests/golden/scan_op_*.npz,
 * conv_op.npz) and against oracle_model.selective_scan.
 *
 * Layout: batch-major like the reference: u, delta, z, out (b, E, L); A (E, N); B, C (b, N, L); D, bias (E).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

static inline float softplusf(float x) { return x > 20.f ? x : log1pf(expf(x)); }
static inline float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

int cad_oracle_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* out = (sum_n C_n h_n + D u) * silu(z),  h_l = exp(dt_l A) h_{l-1} + dt_l B_l u_l,  dt = softplus(delta + bias) */
void cad_oracle_scan_fwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                         const float* D, const float* z, const float* bias, float* out, int64_t nb, int64_t E,
                         int64_t L, int64_t N) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < E; ++e) {
            float h[64];
            for (int64_t n = 0; n < N; ++n) h[n] = 0.f;
            const float* ur = u + (b * E + e) * L;
            const float* dr = delta + (b * E + e) * L;
            const float* zr = z ? z + (b * E + e) * L : NULL;
            float* orow = out + (b * E + e) * L;
            for (int64_t l = 0; l < L; ++l) {
                const float dt = softplusf(dr[l] + (bias ? bias[e] : 0.f));
                float y = 0.f;
                for (int64_t n = 0; n < N; ++n) {
                    h[n] = expf(dt * A[e * N + n]) * h[n] + dt * Bm[(b * N + n) * L + l] * ur[l];
                    y += h[n] * Cm[(b * N + n) * L + l];
                }
                y += (D ? D[e] : 0.f) * ur[l];
                if (zr) y *= zr[l] * sigmoidf(zr[l]);
                orow[l] = y;
            }
        }
}

/* Gradients of the above.  dB, dC are reduced over channels through per-thread buffers (deterministic given the
 * thread count).  All gradient outputs are overwritten. */
void cad_oracle_scan_bwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                         const float* D, const float* z, const float* bias, const float* dout, float* du,
                         float* ddelta, float* dA, float* dB, float* dC, float* dD, float* dz, float* dbias,
                         int64_t nb, int64_t E, int64_t L, int64_t N) {
    const int nt = cad_oracle_num_threads();
    float* dBt = (float*)calloc((size_t)nt * nb * N * L, sizeof(float));
    float* dCt = (float*)calloc((size_t)nt * nb * N * L, sizeof(float));
    float* dAt = (float*)calloc((size_t)nt * E * N, sizeof(float));
    float* dDt = (float*)calloc((size_t)nt * E, sizeof(float));
    float* dbt = (float*)calloc((size_t)nt * E, sizeof(float));
#pragma omp parallel
    {
#ifdef _OPENMP
        const int tid = omp_get_thread_num();
#else
        const int tid = 0;
#endif
        float* hs = (float*)malloc((size_t)(L + 1) * N * sizeof(float)); /* h_{-1..L-1} */
        float* as = (float*)malloc((size_t)L * N * sizeof(float));
        float* dts = (float*)malloc((size_t)L * sizeof(float));
        float* dBp = dBt + (size_t)tid * nb * N * L;
        float* dCp = dCt + (size_t)tid * nb * N * L;
#pragma omp for collapse(2) schedule(static)
        for (int64_t b = 0; b < nb; ++b)
            for (int64_t e = 0; e < E; ++e) {
                const int64_t ro = (b * E + e) * L;
                const float bi = bias ? bias[e] : 0.f, Dv = D ? D[e] : 0.f;
                for (int64_t n = 0; n < N; ++n) hs[n] = 0.f;
                for (int64_t l = 0; l < L; ++l) {
                    const float dt = softplusf(delta[ro + l] + bi);
                    dts[l] = dt;
                    for (int64_t n = 0; n < N; ++n) {
                        const float a = expf(dt * A[e * N + n]);
                        as[l * N + n] = a;
                        hs[(l + 1) * N + n] = a * hs[l * N + n] + dt * Bm[(b * N + n) * L + l] * u[ro + l];
                    }
                }
                float G[64];
                for (int64_t n = 0; n < N; ++n) G[n] = 0.f;
                for (int64_t l = L - 1; l >= 0; --l) {
                    float y = Dv * u[ro + l];
                    for (int64_t n = 0; n < N; ++n) y += hs[(l + 1) * N + n] * Cm[(b * N + n) * L + l];
                    float dy = dout[ro + l];
                    if (z) {
                        const float zz = z[ro + l], sg = sigmoidf(zz);
                        dz[ro + l] = dy * y * sg * (1.f + zz * (1.f - sg));
                        dy *= zz * sg;
                    }
                    const float dt = dts[l], uu = u[ro + l];
                    float ddt = 0.f, ddu = dy * Dv;
                    dDt[(size_t)tid * E + e] += dy * uu;
                    for (int64_t n = 0; n < N; ++n) {
                        const float a = as[l * N + n], Bv = Bm[(b * N + n) * L + l], Cv = Cm[(b * N + n) * L + l];
                        const float g = Cv * dy + G[n];
                        G[n] = a * g;
                        const float t = g * hs[l * N + n] * a;
                        ddt += t * A[e * N + n] + uu * g * Bv;
                        ddu += dt * g * Bv;
                        dAt[((size_t)tid * E + e) * N + n] += t * dt;
                        dBp[(b * N + n) * L + l] += g * dt * uu;
                        dCp[(b * N + n) * L + l] += dy * hs[(l + 1) * N + n];
                    }
                    const float xr = delta[ro + l] + bi;
                    const float dd = ddt * (xr > 20.f ? 1.f : sigmoidf(xr));
                    ddelta[ro + l] = dd;
                    du[ro + l] = ddu;
                    dbt[(size_t)tid * E + e] += dd;
                }
            }
        free(hs);
        free(as);
        free(dts);
    }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nb * N * L; ++i) {
        float sb = 0.f, sc = 0.f;
        for (int t = 0; t < nt; ++t) {
            sb += dBt[(size_t)t * nb * N * L + i];
            sc += dCt[(size_t)t * nb * N * L + i];
        }
        dB[i] = sb;
        dC[i] = sc;
    }
    for (int64_t i = 0; i < E * N; ++i) {
        float s = 0.f;
        for (int t = 0; t < nt; ++t) s += dAt[(size_t)t * E * N + i];
        dA[i] = s;
    }
    for (int64_t i = 0; i < E; ++i) {
        float s1 = 0.f, s2 = 0.f;
        for (int t = 0; t < nt; ++t) {
            s1 += dDt[(size_t)t * E + i];
            s2 += dbt[(size_t)t * E + i];
        }
        if (dD) dD[i] = s1;
        if (dbias) dbias[i] = s2;
    }
    free(dBt);
    free(dCt);
    free(dAt);
    free(dDt);
    free(dbt);
}

/* out[l] = silu(bias + sum_k w[k] x[l-(K-1)+k]);  x, out: (b, E, L); w: (E, K) */
void cad_oracle_conv_fwd(const float* x, const float* w, const float* bias, float* out, int64_t nb, int64_t E,
                         int64_t L, int64_t K) {
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t b = 0; b < nb; ++b)
        for (int64_t e = 0; e < E; ++e) {
            const float* xr = x + (b * E + e) * L;
            float* orow = out + (b * E + e) * L;
            for (int64_t l = 0; l < L; ++l) {
                float acc = bias ? bias[e] : 0.f;
                for (int64_t k = 0; k < K; ++k) {
                    const int64_t j = l - (K - 1) + k;
                    if (j >= 0) acc += w[e * K + k] * xr[j];
                }
                orow[l] = acc * sigmoidf(acc);
            }
        }
}

/* fp64 scan backward for the dB / dC fold checks (tests/test_scan_bwd_sums.py).  Kernel layout: u, delta, z, dout (E, SB, L); B, C
 * (N, SB, L); A (E, N); D, bias (E); rev[SB]: row sb runs from its last position to its first.  delta_is_dt: delta holds dt itself
 * (bias not added), and ddelta / d(bias) are still the gradients w.r.t. the raw delta, d(dt) (1 - exp(-dt)).  The channels are summed
 * the way cad_scan_bwd_multi groups them: slot g holds channels g W .. g W + W - 1.  Outputs, all overwritten:
 *   dB_*, dC_* (N, SB, L): S = sum_e p_e, Ag = sum_g |sum_{e in g} p_e|, Ae = sum_e |p_e|;
 *   dA, dA_abs (E, N), dD, dD_abs, db, db_abs (E): the sums over rows and positions and the sums of the absolute values of their terms;
 *   du, ddelta, dz (E, SB, L): plain values (dz: this set's gate gradient, dout * y * silu'(z); NULL without a gate);
 *   Pg_B, Pg_C, PgA_B, PgA_C (G, N, SB, L): optional (NULL = not wanted), the per-slot sums and their sums of |p_e|.
 * Parallel over the groups of one row at a time; every thread keeps its group's sums for one row (O(threads N L) memory).
 * Returns 0, or -1 if a scratch allocation failed. */
int cad_oracle_scan_bwd_sums_f64(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                                 const float* D, const float* z, const float* bias, const float* dout, const int* rev,
                                 int delta_is_dt, int64_t SB, int64_t E, int64_t L, int64_t N, int64_t W,
                                 double* dB_S, double* dB_Ag, double* dB_Ae, double* dC_S, double* dC_Ag, double* dC_Ae,
                                 double* dA, double* dA_abs, double* dD, double* dD_abs, double* db, double* db_abs,
                                 float* du, float* ddelta, float* dz, double* Pg_B, double* Pg_C,
                                 double* PgA_B, double* PgA_C) {
    const int64_t G = (E + W - 1) / W, NL = N * L;
    const int nt = cad_oracle_num_threads();
    double* scr = (double*)malloc((size_t)nt * 4 * NL * sizeof(double));  /* per thread: P_B, |p|_B, P_C, |p|_C of its group */
    int fail = scr == NULL;
    memset(dA, 0, (size_t)E * N * sizeof(double));
    memset(dA_abs, 0, (size_t)E * N * sizeof(double));
    for (int64_t e = 0; e < E; ++e) dD[e] = dD_abs[e] = db[e] = db_abs[e] = 0.0;
    for (int64_t sb = 0; sb < SB && !fail; ++sb)
        for (int64_t gb = 0; gb < G && !fail; gb += nt) {
            const int64_t ng = G - gb < nt ? G - gb : nt;
#pragma omp parallel
            {
#ifdef _OPENMP
                const int tid = omp_get_thread_num();
#else
                const int tid = 0;
#endif
                const int64_t g = gb + tid;
                double* hs = (double*)malloc((size_t)(L + 1) * N * sizeof(double)); /* h before / after each logical step */
                double* as = (double*)malloc((size_t)L * N * sizeof(double));
                double* dts = (double*)malloc((size_t)L * sizeof(double));
                if (!hs || !as || !dts) {
#pragma omp atomic write
                    fail = 1;
                }
                if (g < G && hs && as && dts) {
                    double* PB = scr + (size_t)tid * 4 * NL;
                    double *AB = PB + NL, *PC = PB + 2 * NL, *AC = PB + 3 * NL;
                    memset(PB, 0, (size_t)4 * NL * sizeof(double));
                    const int64_t e1 = (g + 1) * W < E ? (g + 1) * W : E;
                    for (int64_t e = g * W; e < e1; ++e) {
                        const int64_t ro = (e * SB + sb) * L;
                        const double bi = bias ? bias[e] : 0.0, Dv = D ? D[e] : 0.0;
                        for (int64_t n = 0; n < N; ++n) hs[n] = 0.0;
                        for (int64_t l = 0; l < L; ++l) {
                            const int64_t p = rev[sb] ? L - 1 - l : l;
                            const double x = (double)delta[ro + p] + (delta_is_dt ? 0.0 : bi);
                            const double dt = delta_is_dt ? x : (x > 20.0 ? x : log1p(exp(x)));
                            dts[l] = dt;
                            for (int64_t n = 0; n < N; ++n) {
                                const double a = exp(dt * (double)A[e * N + n]);
                                as[l * N + n] = a;
                                hs[(l + 1) * N + n] = a * hs[l * N + n] + dt * (double)Bm[(n * SB + sb) * L + p] * (double)u[ro + p];
                            }
                        }
                        double Gs[64];
                        for (int64_t n = 0; n < N; ++n) Gs[n] = 0.0;
                        double sD = 0.0, sDa = 0.0, sb_ = 0.0, sba = 0.0;
                        for (int64_t l = L - 1; l >= 0; --l) {
                            const int64_t p = rev[sb] ? L - 1 - l : l;
                            const double uu = u[ro + p], dt = dts[l];
                            double dy = dout[ro + p];
                            if (z) {
                                double y = Dv * uu;
                                for (int64_t n = 0; n < N; ++n) y += hs[(l + 1) * N + n] * (double)Cm[(n * SB + sb) * L + p];
                                const double zz = z[ro + p], sg = 1.0 / (1.0 + exp(-zz));
                                dz[ro + p] = (float)(dy * y * sg * (1.0 + zz * (1.0 - sg)));
                                dy *= zz * sg;
                            }
                            double ddt = 0.0, ddu = dy * Dv;
                            sD += dy * uu;
                            sDa += fabs(dy * uu);
                            for (int64_t n = 0; n < N; ++n) {
                                const double a = as[l * N + n], Bv = Bm[(n * SB + sb) * L + p], Cv = Cm[(n * SB + sb) * L + p];
                                const double gg = Cv * dy + Gs[n];
                                Gs[n] = a * gg;
                                const double t = gg * hs[l * N + n] * a;
                                ddt += t * (double)A[e * N + n] + uu * gg * Bv;
                                ddu += dt * gg * Bv;
                                dA[e * N + n] += t * dt;
                                dA_abs[e * N + n] += fabs(t * dt);
                                const double pb = gg * dt * uu, pc = dy * hs[(l + 1) * N + n];
                                PB[n * L + p] += pb;
                                AB[n * L + p] += fabs(pb);
                                PC[n * L + p] += pc;
                                AC[n * L + p] += fabs(pc);
                            }
                            double sig;
                            if (delta_is_dt) {
                                sig = -expm1(-dt);
                            } else {
                                const double x = (double)delta[ro + p] + bi;
                                sig = 1.0 / (1.0 + exp(-x));
                            }
                            const double dd = ddt * sig;
                            ddelta[ro + p] = (float)dd;
                            du[ro + p] = (float)ddu;
                            sb_ += dd;
                            sba += fabs(dd);
                        }
                        dD[e] += sD, dD_abs[e] += sDa, db[e] += sb_, db_abs[e] += sba;
                    }
                }
                free(hs);
                free(as);
                free(dts);
#pragma omp barrier
                /* fold this batch of groups into the row's sums (fixed order: deterministic) */
#pragma omp for schedule(static)
                for (int64_t i = 0; i < NL; ++i) {
                    const int64_t n = i / L, p = i % L, o = (n * SB + sb) * L + p;
                    double sB = gb ? dB_S[o] : 0.0, gB = gb ? dB_Ag[o] : 0.0, eB = gb ? dB_Ae[o] : 0.0;
                    double sC = gb ? dC_S[o] : 0.0, gC = gb ? dC_Ag[o] : 0.0, eC = gb ? dC_Ae[o] : 0.0;
                    for (int64_t t = 0; t < ng; ++t) {
                        const double* P = scr + (size_t)t * 4 * NL;
                        sB += P[i], gB += fabs(P[i]), eB += P[NL + i];
                        sC += P[2 * NL + i], gC += fabs(P[2 * NL + i]), eC += P[3 * NL + i];
                        if (Pg_B) Pg_B[((gb + t) * N + n) * SB * L + sb * L + p] = P[i];
                        if (Pg_C) Pg_C[((gb + t) * N + n) * SB * L + sb * L + p] = P[2 * NL + i];
                        if (PgA_B) PgA_B[((gb + t) * N + n) * SB * L + sb * L + p] = P[NL + i];
                        if (PgA_C) PgA_C[((gb + t) * N + n) * SB * L + sb * L + p] = P[3 * NL + i];
                    }
                    dB_S[o] = sB, dB_Ag[o] = gB, dB_Ae[o] = eB;
                    dC_S[o] = sC, dC_Ag[o] = gC, dC_Ae[o] = eC;
                }
            }
        }
    free(scr);
    return fail ? -1 : 0;
}
