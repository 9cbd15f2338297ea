// Resampling in time by a rational factor (resample.py, dataset/resident.py: DATA.source_rate): a polyphase FIR over
// lead-major rows of a device buffer.  Definition: include/nefnet_hip.h (nef_resample_args).
//
// nef_resample   one workgroup per (table row, lead, tile of 1024 outputs).  The input stretch the tile's windows cover is staged in LDS
//                once, clamped to the row (edge replication), as fp32 -- the stored int16 / fp32 values survive that exactly; a thread takes
//                groups of 8 positions through load8.  Each thread then forms four outputs, tile0 + lane + 256 j: phase p and first
//                input from one 32-bit division, the K products summed in fp64 in ascending order.  The taps [up, K] come from LDS when
//                up * K <= 4096 doubles and from global memory otherwise; same order, same bits.  A tile whose stretch would not fit
//                the staging array (down / up above ~7) is worked in two halves, each staged once.
//
// The kernel trusts neither table: a row that leaves a buffer writes nothing, and an output whose window -- as `first` places it -- is not
// inside the staged stretch reads its clamped samples from global memory instead, which gives the same sum.  No state, no atomics, no
// scratch, one writer per element.  -ffp-contract=off keeps every multiply and add separately rounded.
#include "nef_common.h"
#include "beat_io.h"

namespace {

constexpr int TILE = NEF_RESAMPLE_TILE;
constexpr int LDS_TAPS = NEF_RESAMPLE_LDS_TAPS;
constexpr int STRETCH = 8000;               // staged samples; with the taps: 32 000 + 32 768 bytes of LDS
static_assert(TILE == 4 * 256, "a thread owns 4 outputs of a tile");
static_assert(STRETCH % 8 == 0, "staging goes in groups of 8");
static_assert((TILE / 2 - 1) * NEF_RESAMPLE_MAX_RATIO + 3 + NEF_RESAMPLE_MAX_K <= STRETCH, "half a tile always fits");

// a table row (in_offset, len, out_offset, rows) that stays inside both buffers and inside the launch's extents; gives its out_len
__device__ __forceinline__ bool resample_row_ok(const int64_t* __restrict__ row, const nef_resample_args& a, int64_t& out_len) {
    const int64_t off = row[0], len = row[1], ooff = row[2], rows = row[3];
    out_len = 0;
    if (!(len >= 1 && len <= 0x7FFF0000ll && rows >= 1 && rows <= a.max_rows && off >= 0 && ooff >= 0)) return false;
    out_len = (len * a.up + a.down - 1) / a.down;
    return out_len >= 1 && out_len <= a.max_out_len && len <= a.src_elems / rows && off <= a.src_elems - rows * len &&
           out_len <= a.dst_elems / rows && ooff <= a.dst_elems - rows * out_len;
}

template <typename T, bool TAPS_IN_LDS>
__global__ __launch_bounds__(256) void resample_kernel(const nef_resample_args a) {
    __shared__ double tap_s[TAPS_IN_LDS ? LDS_TAPS : 1];
    __shared__ float xs[STRETCH];
    __shared__ int fmin_s[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* __restrict__ row = a.table + 4 * (int64_t)blockIdx.z;
    int64_t out_len64;
    if (!resample_row_ok(row, a, out_len64)) return;                                    // block-uniform
    const int lead = (int)blockIdx.y;
    if (lead >= row[3]) return;                                                         // block-uniform
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= out_len64) return;                                                        // block-uniform
    const int len = (int)row[1], up = a.up, down = a.down, K = a.K;
    const int n_out = out_len64 - t0 < TILE ? (int)(out_len64 - t0) : TILE;             // outputs of this tile
    const int64_t base = row[0] + (int64_t)lead * len;
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.src) + base;
    float* __restrict__ dst = a.dst + row[2] + (int64_t)lead * out_len64 + t0;
    const double* __restrict__ taps = a.taps;
    const int32_t* __restrict__ first = a.first;

    // ---- the taps, and the smallest entry of `first`: where the staged stretch starts
    if (TAPS_IN_LDS)
        for (int i = tid; i < up * K; i += 256) tap_s[i] = taps[i];
    int fm = 0x7FFFFFFF;
    for (int p = tid; p < up; p += 256) {
        const int f = first[p];
        fm = f < fm ? f : fm;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(fm, o, 64);
        fm = w < fm ? w : fm;
    }
    if (lane == 0) fmin_s[wave] = fm;
    __syncthreads();
    fm = fmin_s[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) fm = fmin_s[w] < fm ? fmin_s[w] : fm;

    // output t0 + l reads from input q0 + (r0 + l down) / up + first[p] on, p = (r0 + l down) % up; r0 + l down < 2^24
    const int64_t q0 = t0 * down / up;
    const unsigned r0 = (unsigned)(t0 * down % up);
    // a part of S outputs spans at most (S - 1) down / up + 1 inputs between its first and last window
    const int S = (TILE - 1) * down / up + 3 + K <= STRETCH ? TILE : TILE / 2;

    for (int l0 = 0; l0 < n_out; l0 += S) {                                             // block-uniform trip count
        const int l1 = (l0 + S < n_out ? l0 + S : n_out) - 1;                           // the last output of this part
        const int64_t b = q0 + (r0 + (unsigned)l0 * (unsigned)down) / (unsigned)up + fm;
        const int span = (int)((r0 + (unsigned)l1 * (unsigned)down) / (unsigned)up - (r0 + (unsigned)l0 * (unsigned)down) / (unsigned)up) + 2 + K;
        if (l0) __syncthreads();                                                        // the part before is done with xs
        // ---- x[clamp(b + j)] for j in [0, span), a group of 8 positions a thread; span <= STRETCH by the choice of S
        for (int g = tid; 8 * g < span; g += 256) {
            const int64_t u0 = b + 8 * g;
            double x[8];
            if (u0 >= 0 && u0 + 8 <= len) {
                load8(sig + u0, 8, elem_align<T>(base + u0), x);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int64_t q = u0 + i;
                    x[i] = (double)sig[q < 0 ? 0 : (q > len - 1 ? len - 1 : q)];
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) xs[8 * g + i] = (float)x[i];                    // exact: x came from an int16 or a float
        }
        __syncthreads();

        // ---- the outputs: ascending k from +0.0
        for (int l = l0 + tid; l <= l1; l += 256) {
            const unsigned v = r0 + (unsigned)l * (unsigned)down;
            const int p = (int)(v % (unsigned)up);
            const int64_t i0 = q0 + v / (unsigned)up + first[p];
            const int64_t lo = i0 - b;
            const double* __restrict__ tp = (TAPS_IN_LDS ? tap_s : taps) + p * K;
            double s = 0.0;
            if (lo >= 0 && lo + K <= span) {
                const float* __restrict__ xp = xs + (int)lo;
                for (int k = 0; k < K; ++k) s = s + tp[k] * (double)xp[k];
            } else {                                                                    // a `first` no design gives: the formula, from global memory
                for (int k = 0; k < K; ++k) {
                    const int64_t q = i0 + k;
                    s = s + tp[k] * (double)sig[q < 0 ? 0 : (q > len - 1 ? len - 1 : q)];
                }
            }
            dst[l] = (float)s;
        }
    }
}

}  // namespace

extern "C" {

size_t nef_resample_args_bytes(void) { return sizeof(nef_resample_args); }

int nef_resample(const nef_resample_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->src && a->table && a->dst && a->taps && a->first, NEF_E_NULL);
    NEF_REQUIRE(a->N >= 1 && a->N <= 65535 && a->max_rows >= 1 && a->max_rows <= 65535 && a->max_out_len >= 1 && a->max_out_len <= 0x7FFF0000ll,
                NEF_E_SHAPE);
    NEF_REQUIRE(a->up >= 1 && a->up <= NEF_RESAMPLE_MAX_UP && a->K >= 1 && a->K <= NEF_RESAMPLE_MAX_K && a->down >= 1 &&
                a->down <= NEF_RESAMPLE_MAX_RATIO * a->up, NEF_E_SHAPE);
    NEF_REQUIRE((a->dtype == 0 || a->dtype == 1) && a->src_elems >= 1 && a->src_elems < (1ll << 56) && a->dst_elems >= 1 &&
                a->dst_elems < (1ll << 56), NEF_E_SHAPE);
    NEF_REQUIRE(((uintptr_t)a->src & 15) == 0 && (((uintptr_t)a->table | (uintptr_t)a->taps) & 7) == 0 &&
                (((uintptr_t)a->dst | (uintptr_t)a->first) & 3) == 0, NEF_E_UNSUPPORTED);
    const dim3 grid((unsigned)nef_cdiv(a->max_out_len, TILE), (unsigned)a->max_rows, (unsigned)a->N);
    const bool lds = a->up * a->K <= LDS_TAPS;
    if (a->dtype == 0) {
        if (lds)
            hipLaunchKernelGGL((resample_kernel<int16_t, true>), grid, dim3(256), 0, (hipStream_t)stream, *a);
        else
            hipLaunchKernelGGL((resample_kernel<int16_t, false>), grid, dim3(256), 0, (hipStream_t)stream, *a);
    } else {
        if (lds)
            hipLaunchKernelGGL((resample_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, *a);
        else
            hipLaunchKernelGGL((resample_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, *a);
    }
    return nef_launch_status();
}

}  // extern "C"
