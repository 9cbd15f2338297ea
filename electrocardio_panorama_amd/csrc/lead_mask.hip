// Lead masks (cfg.MODEL.lead_mask): the lead mean, the Standin mixes and their adjoint over each sample's PRESENT leads, and the mask
// that says which rows nef_augment dropped.  Definition: include/nefnet_hip.h (nef_lead_mask_mix_fwd_args and the two behind it).
//
// Both mix kernels give one wave a (sample, channel) row, as lead_mean_kernel / mix_fwd_kernel / mix_bwd_kernel do.  The sample's mask
// row (V <= 12 bytes) is decoded once per row into a wave-uniform bit set; the lead loop walks its set bits in ascending order with
// scalar instructions, so absent leads cost no load and the inner loop has no per-element branch on v.  A row of every tensor involved
// starts (c T mod 4) floats behind a 16-byte boundary -- a sample's or a lead's rows are 128 T or 256 T floats, a multiple of 4 -- so
// with 16-byte aligned bases a row is cut into a head of up to three single elements, 16-byte vectors and a tail of single elements, the
// same for every tensor.  The expressions per element are those of the kernels named above on every path.  No atomics, one writer per
// element, no LDS, no scratch.
#include "nef_common.h"
#include "aug_drop.h"
#include "up2_adjoint.h"

namespace {

// the mask row of sample b as a bit set (bit v: lead v is present), the same in every lane
__device__ __forceinline__ uint32_t present_bits(const uint8_t* __restrict__ mask, int b, int V) {
    uint32_t bits = 0;
    for (int v = 0; v < V; ++v) bits |= (mask[(int64_t)b * V + v] != 0 ? 1u : 0u) << v;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)bits);
}

// P_b[c mod n_b] for n_b > 0: the (c mod n_b)-th set bit from below
__device__ __forceinline__ int pick_lead(uint32_t bits, int n, int c) {
    for (uint32_t k = (uint32_t)c % (uint32_t)n; k; --k) bits &= bits - 1;
    return __builtin_ctz(bits);
}

// elements of the row in front of its first 16-byte boundary (0 when the row is handled element by element)
__device__ __forceinline__ int row_head(int cc, int T, int vec) {
    if (!vec) return T;
    const int h = (4 - ((cc * T) & 3)) & 3;      // cc < 128, T <= 2^24
    return h < T ? h : T;
}

// W consecutive positions from t of G column groups 64 W apart: every present lead is read once, G W loads in flight per lead
template <int W, int G>
__device__ __forceinline__ void fwd_elems(const float* __restrict__ src, int64_t lead, uint32_t bits, int pv, float fn, float f, bool first,
                                          float* __restrict__ lat, float* __restrict__ d0, int64_t pass, int t) {
    typedef float vec __attribute__((ext_vector_type(W)));
    uint32_t m = bits;
    int v = __builtin_ctz(m);
    m &= m - 1;
    vec s[G], pk[G];
#pragma unroll
    for (int g = 0; g < G; ++g) pk[g] = s[g] = *(const vec*)(src + (int64_t)v * lead + t + g * 64 * W);
    while (m) {
        v = __builtin_ctz(m);
        m &= m - 1;
        vec x[G];
#pragma unroll
        for (int g = 0; g < G; ++g) x[g] = *(const vec*)(src + (int64_t)v * lead + t + g * 64 * W);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            s[g] += x[g];
            if (v == pv) pk[g] = x[g];      // wave-uniform
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int tg = t + g * 64 * W;
        const vec mean = s[g] / fn;
        *(vec*)(lat + tg) = mean;
        if (d0) {
            *(vec*)(d0 + tg) = f * mean;
            *(vec*)(d0 + pass + tg) = f * (first ? pk[g] : mean);
            *(vec*)(d0 + 2 * pass + tg) = f * (first ? mean : pk[g]);
        }
    }
}

template <int W>
__device__ __forceinline__ void zero_elems(float* __restrict__ p, int t) {
    typedef float vec __attribute__((ext_vector_type(W)));
    *(vec*)(p + t) = (vec)(0.f);
}

__global__ __launch_bounds__(256) void lead_mask_mix_fwd_kernel(const nef_lead_mask_mix_fwd_args a, int vec) {
    int c1 = a.c1, c2 = a.c2;
    if (a.choice_dev) { c1 = a.choice_dev[0]; c2 = a.choice_dev[1]; }      // graph replay: the Standin draw lives on the device
    const int B = a.B, V = a.V, T = a.T;
    const int64_t rows = (int64_t)B * 256;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t pass = rows * T, lead = (int64_t)128 * T;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = __builtin_amdgcn_readfirstlane((int)(row >> 8)), c = __builtin_amdgcn_readfirstlane((int)(row & 255));
        const bool first = c < 128;
        const int cc = c & 127;
        const uint32_t bits = present_bits(a.mask, b, V);
        const int n = __builtin_popcount(bits);
        float* __restrict__ lat = a.latent + row * T;
        float* __restrict__ d0 = a.D ? a.D + row * T : nullptr;
        const int head = row_head(cc, T, vec);
        const int nv = (T - head) >> 2, tail0 = head + 4 * nv;
        if (c == 0 && lane == 0 && a.picks) {
            a.picks[2 * b] = n ? pick_lead(bits, n, c1) : -1;
            a.picks[2 * b + 1] = n ? pick_lead(bits, n, c2) : -1;
        }
        if (n == 0) {      // no present lead: exact zeros, nothing is read
            for (int t = lane; t < head; t += 64) {
                zero_elems<1>(lat, t);
                if (d0) { zero_elems<1>(d0, t); zero_elems<1>(d0 + pass, t); zero_elems<1>(d0 + 2 * pass, t); }
            }
            for (int i = lane; i < nv; i += 64) {
                zero_elems<4>(lat, head + 4 * i);
                if (d0) { zero_elems<4>(d0, head + 4 * i); zero_elems<4>(d0 + pass, head + 4 * i); zero_elems<4>(d0 + 2 * pass, head + 4 * i); }
            }
            for (int t = tail0 + lane; t < T; t += 64) {
                zero_elems<1>(lat, t);
                if (d0) { zero_elems<1>(d0, t); zero_elems<1>(d0 + pass, t); zero_elems<1>(d0 + 2 * pass, t); }
            }
            continue;
        }
        const int pv = pick_lead(bits, n, first ? c1 : c2);
        const float fn = (float)n;
        const float f = a.q ? a.q[row] : 0.f;
        const float* __restrict__ src = (first ? a.z1 : a.z2r) + ((int64_t)b * V * 128 + cc) * T;
        for (int t = lane; t < head; t += 64) fwd_elems<1, 1>(src, lead, bits, pv, fn, f, first, lat, d0, pass, t);
        int i = lane;
        for (; i + 64 < nv; i += 128) fwd_elems<4, 2>(src, lead, bits, pv, fn, f, first, lat, d0, pass, head + 4 * i);
        for (; i < nv; i += 64) fwd_elems<4, 1>(src, lead, bits, pv, fn, f, first, lat, d0, pass, head + 4 * i);
        for (int t = tail0 + lane; t < T; t += 64) fwd_elems<1, 1>(src, lead, bits, pv, fn, f, first, lat, d0, pass, t);
    }
}

// W consecutive positions from t: returns this lane's share of the row's gq sum
template <int W, bool UP>
__device__ __forceinline__ float bwd_elems(const float* __restrict__ g0, int64_t gpass, const float* __restrict__ lat,
                                           const float* __restrict__ zsrc, float* __restrict__ gdst, int64_t lead, uint32_t bits, int pv,
                                           int V, float fn, float f, bool first, bool relu, int T, int t) {
    typedef float vec __attribute__((ext_vector_type(W)));
    vec ga, gb, gc;
    if constexpr (UP) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            ga[e] = up2_adjoint(g0, T, t + e);
            gb[e] = up2_adjoint(g0 + gpass, T, t + e);
            gc[e] = up2_adjoint(g0 + 2 * gpass, T, t + e);
        }
    } else {
        ga = *(const vec*)(g0 + t);
        gb = *(const vec*)(g0 + gpass + t);
        gc = *(const vec*)(g0 + 2 * gpass + t);
    }
    // pass that uses the picked lead for this half: D1 for the z1 half, D2 for the z2 half
    const vec g_pick = first ? gb : gc;
    const vec g_mean = first ? (ga + gc) : (ga + gb);
    const vec l = *(const vec*)(lat + t);
    const vec pk = *(const vec*)(zsrc + (int64_t)pv * lead + t);
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < W; ++e) acc += g_mean[e] * l[e] + g_pick[e] * pk[e];
    const vec gm = f * g_mean / fn;
    const vec gp = f * g_pick;
    const vec zero = (vec)(0.f);
    for (int v = 0; v < V; ++v) {      // every row is written; present / picked are wave-uniform
        vec o = zero;
        if ((bits >> v) & 1u) {
            o = gm + (v == pv ? gp : zero);
            if (relu) {                // z1 is a ReLU output: its backward mask is taken here (present leads only are read)
                const vec z = *(const vec*)(zsrc + (int64_t)v * lead + t);
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (!(z[e] > 0.f)) o[e] = 0.f;
            }
        }
        *(vec*)(gdst + (int64_t)v * lead + t) = o;
    }
    return acc;
}

template <bool UP>
__global__ __launch_bounds__(256) void lead_mask_mix_bwd_kernel(const nef_lead_mask_mix_bwd_args a, int vec) {
    int c1 = a.c1, c2 = a.c2;
    if (a.choice_dev) { c1 = a.choice_dev[0]; c2 = a.choice_dev[1]; }
    const int B = a.B, V = a.V, T = a.T;
    const int64_t rows = (int64_t)B * 256;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t pass = rows * T, lead = (int64_t)128 * T;
    const int64_t gpass = UP ? 2 * pass : pass;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = __builtin_amdgcn_readfirstlane((int)(row >> 8)), c = __builtin_amdgcn_readfirstlane((int)(row & 255));
        const bool first = c < 128;
        const int cc = c & 127;
        const uint32_t bits = present_bits(a.mask, b, V);
        const int n = __builtin_popcount(bits);
        float* __restrict__ gdst = (first ? a.gz1 : a.gz2r) + ((int64_t)b * V * 128 + cc) * T;
        const int head = row_head(cc, T, vec);
        const int nv = (T - head) >> 2, tail0 = head + 4 * nv;
        if (n == 0) {      // no present lead: exact zeros, nothing is read
            for (int v = 0; v < V; ++v) {
                float* __restrict__ gr = gdst + (int64_t)v * lead;
                for (int t = lane; t < head; t += 64) zero_elems<1>(gr, t);
                for (int i = lane; i < nv; i += 64) zero_elems<4>(gr, head + 4 * i);
                for (int t = tail0 + lane; t < T; t += 64) zero_elems<1>(gr, t);
            }
            if (lane == 0) a.gq[row] = 0.f;
            continue;
        }
        const int pv = pick_lead(bits, n, first ? c1 : c2);
        const float fn = (float)n;
        const float f = a.q[row];
        const bool relu = a.relu_z1 && first;
        const float* __restrict__ lat = a.latent + row * T;
        const float* __restrict__ zsrc = (first ? a.z1 : a.z2r) + ((int64_t)b * V * 128 + cc) * T;
        const float* __restrict__ g0 = a.gD + row * (UP ? 2 * (int64_t)T : (int64_t)T);
        float acc = 0.f;
        for (int t = lane; t < head; t += 64) acc += bwd_elems<1, UP>(g0, gpass, lat, zsrc, gdst, lead, bits, pv, V, fn, f, first, relu, T, t);
        for (int i = lane; i < nv; i += 64)
            acc += bwd_elems<4, UP>(g0, gpass, lat, zsrc, gdst, lead, bits, pv, V, fn, f, first, relu, T, head + 4 * i);
        for (int t = tail0 + lane; t < T; t += 64) acc += bwd_elems<1, UP>(g0, gpass, lat, zsrc, gdst, lead, bits, pv, V, fn, f, first, relu, T, t);
        acc = nef_wave_sum(acc);
        if (lane == 0) a.gq[row] = acc;
    }
}

__global__ __launch_bounds__(256) void augment_mask_kernel(const nef_augment_mask_args a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.B * a.V) return;
    const int b = (int)(i / a.V), v = (int)(i - (int64_t)b * a.V);
    const uint64_t seed = a.seed + (a.seed_dev ? a.seed_dev[0] : 0ull);
    a.mask[i] = nef_aug::lead_dropped(seed, b, v, a.V, a.lead_drop) ? 0 : 1;
}

inline bool al(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// B, V, T of either mix entry
inline bool mix_shape_ok(int B, int V, int T) {
    return B > 0 && V >= 1 && V <= NEF_LEAD_MASK_MAX_V && T >= 1 && T <= (1 << 24) && (int64_t)B * 256 * 6 < ((int64_t)1 << 62) / T;
}

}  // namespace

extern "C" {

size_t nef_lead_mask_mix_fwd_args_bytes(void) { return sizeof(nef_lead_mask_mix_fwd_args); }
size_t nef_lead_mask_mix_bwd_args_bytes(void) { return sizeof(nef_lead_mask_mix_bwd_args); }
size_t nef_augment_mask_args_bytes(void) { return sizeof(nef_augment_mask_args); }

int nef_lead_mask_mix_fwd(const nef_lead_mask_mix_fwd_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->z1 && a->z2r && a->mask && a->latent, NEF_E_NULL);
    NEF_REQUIRE((a->q == nullptr) == (a->D == nullptr), NEF_E_NULL);
    NEF_REQUIRE(mix_shape_ok(a->B, a->V, a->T) && a->c1 >= 0 && a->c2 >= 0, NEF_E_SHAPE);
    NEF_REQUIRE(al(a->z1, 4) && al(a->z2r, 4) && al(a->q, 4) && al(a->latent, 4) && al(a->D, 4) && al(a->picks, 4) && al(a->choice_dev, 4),
                NEF_E_UNSUPPORTED);
    const int vec = al(a->z1, 16) && al(a->z2r, 16) && al(a->latent, 16) && al(a->D, 16);
    hipLaunchKernelGGL(lead_mask_mix_fwd_kernel, dim3(nef_stream_grid((int64_t)a->B * 256, 4)), dim3(256), 0, (hipStream_t)stream, *a, vec);
    return nef_launch_status();
}

int nef_lead_mask_mix_bwd(const nef_lead_mask_mix_bwd_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->gD && a->latent && a->z1 && a->z2r && a->q && a->mask && a->gz1 && a->gz2r && a->gq, NEF_E_NULL);
    NEF_REQUIRE(mix_shape_ok(a->B, a->V, a->T) && a->c1 >= 0 && a->c2 >= 0, NEF_E_SHAPE);
    NEF_REQUIRE(al(a->gD, 4) && al(a->latent, 4) && al(a->z1, 4) && al(a->z2r, 4) && al(a->q, 4) && al(a->gz1, 4) && al(a->gz2r, 4) &&
                    al(a->gq, 4) && al(a->choice_dev, 4),
                NEF_E_UNSUPPORTED);
    // (up: the 2T-long gradient rows are read element by element through the adjoint, so gD's alignment does not matter there)
    const int vec = al(a->latent, 16) && al(a->z1, 16) && al(a->z2r, 16) && al(a->gz1, 16) && al(a->gz2r, 16) && (a->up || al(a->gD, 16));
    const dim3 grid(nef_stream_grid((int64_t)a->B * 256, 4));
    if (a->up)
        hipLaunchKernelGGL(lead_mask_mix_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *a, vec);
    else
        hipLaunchKernelGGL(lead_mask_mix_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *a, vec);
    return nef_launch_status();
}

int nef_augment_mask(const nef_augment_mask_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->mask, NEF_E_NULL);
    NEF_REQUIRE(a->B > 0 && a->V >= 1 && a->V <= NEF_LEAD_MASK_MAX_V && (int64_t)a->B * a->V <= 0x7FFFFFFFll, NEF_E_SHAPE);
    NEF_REQUIRE(a->lead_drop >= 0.f && a->lead_drop < 1.f, NEF_E_SHAPE);      // (NaN fails both)
    NEF_REQUIRE(al(a->seed_dev, 8), NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(augment_mask_kernel, dim3((unsigned)nef_cdiv((int64_t)a->B * a->V, 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
