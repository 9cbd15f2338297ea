// Heavy-tail census of a split-fp16 operand, and the row-end terms that let an fp32 weight gradient stand in for the split-fp16
// polyphase one (pro_mode bit 2).  Both serve the per-site fp32 route of the split-fp16 weight gradients (ops.H2_TAIL_MODE):
// the census runs once per call-site lifetime, at the site's measuring launch; the row-end pass only on sites that route to fp32.
#include "nef_common.h"

namespace {

constexpr int CENSUS_BLOCK = 256;
constexpr int CENSUS_MAX_GRID = 1024;

// One wave per (b, g, c) row of the view, grid-stride over rows; a lane takes columns lane, lane + 64, ...  Element value = what
// the split-fp16 launch splits: v = x, then max(fma(v, a, b), 0) with a / b [pass = b / Bp][g Cg + c] when pro_mode bit 0 is set,
// then v * in_scale[b sc_bs + g sc_gs + c].  With the x2 upsampling bit the view is the HALF-resolution input and the census counts
// those values, not the interpolated ones the launch forms from them (every interpolated value is a 3:1 / 1:3 blend of two
// neighbours).  The amax the launch measured is the INTERPOLATED operand's, and it can be smaller than the largest half-resolution
// value (an isolated interior spike x[m] interpolates to at most 0.75 x[m], less still between neighbours of the opposite sign):
// v / amax can then exceed 1, which changes no count and only weights the energies.  The clamped-window bit (4) and the polyphase
// bit (8) add no values.
// Per lane: counts in 32-bit words, the squares of v / amax in fp32 over the row; per row the wave sums those in fp32 and adds the
// row's total to fp64 accumulators (no fp64 copy of the operand); per block: one [4] fp64 partial (counts are exact integers).
__global__ __launch_bounds__(CENSUS_BLOCK) void h2_tail_census_partial(const float* __restrict__ x, int64_t x_bs, int64_t x_gs, int B,
                                                                        int G, int Cg, int T, const float* __restrict__ in_scale,
                                                                        int64_t sc_bs, int64_t sc_gs, const float* __restrict__ pro_a,
                                                                        const float* __restrict__ pro_b, int aff, int pro_Bp,
                                                                        const float* __restrict__ amax, float window,
                                                                        double* __restrict__ part) {
    __shared__ double red[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float m = amax[0];
    const bool live = m > 0.f && m < 3.4e38f;
    const float thr = live ? m * window : 0.f, inv = live ? 1.f / m : 0.f;
    double n_nz = 0.0, n_sm = 0.0, e_sm = 0.0, e_all = 0.0;
    const int64_t rows = (int64_t)B * G * Cg;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int c = (int)(row % Cg);
        const int64_t bg = row / Cg;
        const int g = (int)(bg % G), b = (int)(bg / G);
        float pa = 1.f, pb = 0.f, sc = 1.f;
        if (aff) {
            const int64_t pr = (int64_t)(b / pro_Bp) * G * Cg + (int64_t)g * Cg + c;
            pa = pro_a[pr], pb = pro_b[pr];
        }
        if (in_scale) sc = in_scale[(int64_t)b * sc_bs + (int64_t)g * sc_gs + c];
        const float* xr = x + (int64_t)b * x_bs + (int64_t)g * x_gs + (int64_t)c * T;
        unsigned cnz = 0, csm = 0;
        float esm = 0.f, eall = 0.f;
        for (int t0 = 0; t0 < T; t0 += 256) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = t0 + 64 * k + lane;
                v[k] = t < T ? xr[t] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = v[k];
                if (aff) s = fmaxf(fmaf(s, pa, pb), 0.f);
                if (in_scale) s = s * sc;
                // (columns past T hold 0.0 and a zero stays zero through the prologue only without `aff`: mask them explicitly)
                const float a = (t0 + 64 * k + lane < T) ? fabsf(s) : 0.f;
                const bool nz = a > 0.f, sm = nz && a < thr;
                const float q = a * inv, q2 = q * q;
                cnz += nz, csm += sm;
                eall += nz ? q2 : 0.f;
                esm += sm ? q2 : 0.f;
            }
        }
        const float we_all = nef_wave_sum(eall), we_sm = nef_wave_sum(esm);
        const float wn = nef_wave_sum((float)cnz), ws = nef_wave_sum((float)csm);      // <= T: exact in fp32 below 2^24
        n_nz += (double)wn, n_sm += (double)ws, e_all += (double)we_all, e_sm += (double)we_sm;
    }
    if (lane == 0) red[wave][0] = n_nz, red[wave][1] = n_sm, red[wave][2] = e_sm, red[wave][3] = e_all;
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[(int64_t)blockIdx.x * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// One workgroup: the block partials in a fixed order (bitwise reproducible), then the record, the optional site word and the
// optional running maxima of the count / energy fractions (the `tail_stat` diagnostics).
__global__ __launch_bounds__(CENSUS_BLOCK) void h2_tail_census_final(const double* __restrict__ part, int nblk, float frac,
                                                                      nef_h2_tail_census_out* __restrict__ out, int32_t* __restrict__ site_flag,
                                                                      float* __restrict__ stat) {
    __shared__ double sm[4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += CENSUS_BLOCK)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += part[(int64_t)i * 4 + k];
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = nef_block_sum_d(v[k], sm);
    if (threadIdx.x == 0) {
        const double nz = r[0] > 1.0 ? r[0] : 1.0;
        const float cf = (float)(r[1] / nz);
        const float ef = r[3] > 0.0 ? (float)(r[2] / r[3]) : 0.f;
        const int flag = cf > frac ? 1 : 0;
        out->n_nonzero = (uint64_t)r[0];
        out->n_small = (uint64_t)r[1];
        out->e_small = r[2];
        out->e_total = r[3];
        out->frac_count = cf;
        out->frac_energy = ef;
        out->flag = flag;
        out->reserved = 0;
        if (site_flag && flag) site_flag[0] = 1;
        if (stat) {
            stat[0] = fmaxf(stat[0], cf);
            stat[1] = fmaxf(stat[1], ef);
        }
    }
}

// gw[r][ci][0] += sum_b gy[b][r][0] xedge[b][ci][0],  gw[r][ci][2] += sum_b gy[b][r][T-1] xedge[b][ci][1]  (K = 3, rows r of group
// g; xedge = the prologue's output x' at both row ends).  What a K = 3 weight gradient over a window continued with x'[0] / x'[T-1]
// (instead of zeros) at both row ends adds to the zero-padded one: tap 0 of output column 0 reads column -1, tap 2 of the last
// column reads column T.  CE_ROWS rows per workgroup share the xedge loads; samples in order (no atomics, reproducible).
constexpr int CE_ROWS = 16;
__global__ __launch_bounds__(256) void bwd_weight_clamp_ends_kernel(const float* __restrict__ xedge, const float* __restrict__ gy,
                                                                    int64_t gy_bs, int64_t gy_gs, float* __restrict__ gw, int B, int T,
                                                                    int G, int Cig, int Cog) {
    __shared__ float ge[2][64][CE_ROWS];
    const int rb = Cog / CE_ROWS;
    const int g = blockIdx.x / rb, r0 = (blockIdx.x - g * rb) * CE_ROWS;
    for (int ci0 = 0; ci0 < Cig; ci0 += 256) {
        const int ci = ci0 + threadIdx.x;
        float s0[CE_ROWS], s1[CE_ROWS];
#pragma unroll
        for (int r = 0; r < CE_ROWS; ++r) s0[r] = 0.f, s1[r] = 0.f;
        for (int b0 = 0; b0 < B; b0 += 64) {
            const int nb = B - b0 < 64 ? B - b0 : 64;
            __syncthreads();
            for (int i = threadIdx.x; i < 2 * 64 * CE_ROWS; i += 256) {
                const int p = i / (64 * CE_ROWS), bi = (i / CE_ROWS) % 64, r = i % CE_ROWS;
                ge[p][bi][r] = bi < nb ? gy[(int64_t)(b0 + bi) * gy_bs + (int64_t)g * gy_gs + (int64_t)(r0 + r) * T + (p ? T - 1 : 0)] : 0.f;
            }
            __syncthreads();
            if (ci < Cig) {
                for (int bi = 0; bi < nb; ++bi) {
                    const nef_f32x2 xe = *(const nef_f32x2*)(xedge + (((int64_t)(b0 + bi) * G + g) * Cig + ci) * 2);
#pragma unroll
                    for (int r = 0; r < CE_ROWS; ++r) s0[r] = fmaf(ge[0][bi][r], xe[0], s0[r]), s1[r] = fmaf(ge[1][bi][r], xe[1], s1[r]);
                }
            }
        }
        if (ci < Cig) {
#pragma unroll
            for (int r = 0; r < CE_ROWS; ++r) {
                float* o = gw + ((int64_t)(g * Cog + r0 + r) * Cig + ci) * 3;
                o[0] += s0[r];
                o[2] += s1[r];
            }
        }
    }
}

int census_grid(int B, int G, int Cg) {
    const int64_t g = nef_cdiv((int64_t)B * G * Cg, 4);
    return (int)(g < 1 ? 1 : (g > CENSUS_MAX_GRID ? CENSUS_MAX_GRID : g));
}

}  // namespace

size_t nef_h2_tail_census_ws_bytes(int B, int G, int Cg) {
    if (B <= 0 || G <= 0 || Cg <= 0) return 0;
    return (size_t)census_grid(B, G, Cg) * 4 * sizeof(double);
}

int nef_h2_tail_census(const float* x, int64_t x_bs, int64_t x_gs, int B, int G, int Cg, int T, const float* in_scale, int64_t sc_bs,
                       int64_t sc_gs, const float* pro_a, const float* pro_b, int pro_mode, int pro_Bp, const float* amax, float window,
                       float frac, void* ws, size_t ws_bytes, nef_h2_tail_census_out* out, int32_t* site_flag, float* tail_stat,
                       nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(x && amax && ws && out, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && G > 0 && Cg > 0 && T > 0 && pro_mode >= 0 && window > 0.f, NEF_E_SHAPE);
    const int aff = pro_mode & 1;
    NEF_REQUIRE(!aff || (pro_a && pro_b && pro_Bp > 0), NEF_E_NULL);
    NEF_REQUIRE(ws_bytes >= nef_h2_tail_census_ws_bytes(B, G, Cg), NEF_E_WORKSPACE);
    const int grid = census_grid(B, G, Cg);
    hipLaunchKernelGGL(h2_tail_census_partial, dim3((unsigned)grid), dim3(CENSUS_BLOCK), 0, (hipStream_t)stream, x, x_bs, x_gs, B, G, Cg,
                       T, in_scale, sc_bs, sc_gs, pro_a, pro_b, aff, aff ? pro_Bp : 1, amax, window, (double*)ws);
    hipLaunchKernelGGL(h2_tail_census_final, dim3(1), dim3(CENSUS_BLOCK), 0, (hipStream_t)stream, (const double*)ws, grid, frac, out,
                       site_flag, tail_stat);
    return nef_launch_status();
}

int nef_bwd_weight_clamp_ends(const float* xedge, const float* gy, int64_t gy_bs, int64_t gy_gs, float* gw, int B, int T, int G,
                              int Cin_g, int Cout_g, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(xedge && gy && gw, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && T >= 2 && G > 0 && Cin_g > 0 && Cout_g > 0 && Cout_g % CE_ROWS == 0, NEF_E_SHAPE);
    hipLaunchKernelGGL(bwd_weight_clamp_ends_kernel, dim3((unsigned)(G * (Cout_g / CE_ROWS))), dim3(256), 0, (hipStream_t)stream, xedge,
                       gy, gy_bs, gy_gs, gw, B, T, G, Cin_g, Cout_g);
    return nef_launch_status();
}
