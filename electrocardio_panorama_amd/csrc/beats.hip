// Tianchi batches built from device-resident recordings (cfg.DATA.device_resident): crop one annotated beat, extend its eight stored leads
// by the four derived limb leads, min-max normalise over all 12 leads and pad / crop to 512 samples.  Definition: include/nefnet_hip.h
// (nef_beat_batch_args); the host path whose bits this reproduces: dataset/tianchi.py, EcgTianChiInterval.__getitem__.
//
// One 256-thread workgroup per sample, two passes over the beat.  Pass 1: lo / hi over 12 leads x n positions in fp64 -- work items are
// (lead unit, group of 8 positions); unit 0 reads leads I and II and also forms the four derived leads, units 1..6 read one stored lead each.
// Pass 2 (the beat is in L2 now): a wave owns one output row at a time, a lane 8 positions = two 16-byte stores.  Both passes read a row
// through load8: the widest loads the address of the row's first element allows, element by element otherwise or where the group crosses
// the beat's end; either way the eight values are the stored ones converted to fp64, so nothing depends on the load form.
#include "nef_common.h"

namespace {

constexpr int BL = NEF_BEAT_LEN;
static_assert(BL == 64 * 8, "a wave writes one output row: 8 positions per lane");

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// bytes (16, 8, 4 or 2) to which element e of a 16-byte-aligned buffer of T is aligned
template <typename T>
__device__ __forceinline__ int elem_align(int64_t e) {
    const int a = (int)(((uint64_t)e * sizeof(T)) & 15u);
    return a == 0 ? 16 : (a & -a);
}

// x[i] = p[i] for i < nv (nv in 1..8), 0 behind; p + 8 k keeps p's alignment for every k (8 elements are 16 or 32 bytes)
__device__ __forceinline__ void load8(const int16_t* __restrict__ p, int nv, int align, double (&x)[8]) {
    if (nv == 8 && align >= 4) {
        short v[8];
        if (align == 16) {
            const s16x8 q = *reinterpret_cast<const s16x8*>(p);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = q[i];
        } else if (align == 8) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const s16x4 q = *reinterpret_cast<const s16x4*>(p + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * h + i] = q[i];
            }
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const s16x2 q = *reinterpret_cast<const s16x2*>(p + 2 * h);
                v[2 * h] = q[0];
                v[2 * h + 1] = q[1];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (double)v[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = i < nv ? (double)p[i] : 0.0;
}

__device__ __forceinline__ void load8(const float* __restrict__ p, int nv, int align, double (&x)[8]) {
    if (nv == 8 && align >= 8) {
        float v[8];
        if (align == 16) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(p + 4 * h);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * h + i] = q[i];
            }
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const f32x2 q = *reinterpret_cast<const f32x2*>(p + 2 * h);
                v[2 * h] = q[0];
                v[2 * h + 1] = q[1];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (double)v[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = i < nv ? (double)p[i] : 0.0;
}

// numpy.min / numpy.max: a NaN wins, and stays
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// the four derived limb leads exactly as the host writes them (III, aVR, aVL, aVF); -ffp-contract=off keeps them two roundings each
__device__ __forceinline__ double derived(int which, double i, double ii) {
    return which == 0 ? ii - i : which == 1 ? -0.5 * (i + ii) : which == 2 ? i - 0.5 * ii : ii - 0.5 * i;
}

template <typename T>
__global__ __launch_bounds__(256) void beat_batch_kernel(const nef_beat_batch_args a) {
    __shared__ double red[8];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = a.V + 1 + a.R, W = 3 + rows;
    const int64_t* __restrict__ pl = a.plan + (int64_t)b * W;
    const int64_t off = pl[0], stride = pl[1], n64 = pl[2];

    // the plan row is device data the entry point cannot have seen: a row that leaves `signal` reads nothing (block-uniform)
    bool ok = off >= 0 && off < a.signal_elems && stride >= 1 && stride <= a.signal_elems && n64 >= 1 && n64 <= stride &&
              n64 <= 0x7FFFFFF0ll && off + 7 * stride + n64 <= a.signal_elems;
    for (int r = 0; r < rows; ++r) ok = ok && pl[3 + r] >= 0 && pl[3 + r] < 12;

    float* out_row = nullptr;           // pass 2: this wave's row; 8 positions per lane
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal);
    if (!ok) {
        const float q = __builtin_nanf("");
        for (int r = wave; r < rows; r += 4) {
            out_row = r < a.V ? a.data + ((int64_t)b * a.V + r) * BL : r == a.V ? a.target_view + (int64_t)b * BL
                                                                                 : a.rest_view + ((int64_t)b * a.R + (r - a.V - 1)) * BL;
            reinterpret_cast<f32x4*>(out_row + 8 * lane)[0] = f32x4{q, q, q, q};
            reinterpret_cast<f32x4*>(out_row + 8 * lane)[1] = f32x4{q, q, q, q};
        }
        return;
    }
    const int n = (int)n64;
    const int groups = (n + 7) >> 3;            // <= 2^28: 7 * groups fits an int

    // ---- pass 1: lo, hi
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int it = tid; it < 7 * groups; it += 256) {
        const int unit = it / groups, t0 = (it - unit * groups) * 8;
        const int nv = n - t0 < 8 ? n - t0 : 8;
        double x[8];
        if (unit == 0) {
            double y[8];
            load8(sig + off + t0, nv, elem_align<T>(off), x);
            load8(sig + off + stride + t0, nv, elem_align<T>(off + stride), y);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < nv) {
                    lo = nan_min(nan_min(lo, x[i]), y[i]);
                    hi = nan_max(nan_max(hi, x[i]), y[i]);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const double s = derived(d, x[i], y[i]);
                        lo = nan_min(lo, s);
                        hi = nan_max(hi, s);
                    }
                }
        } else {
            const int64_t e = off + (int64_t)(unit + 1) * stride;
            load8(sig + e + t0, nv, elem_align<T>(e), x);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < nv) {
                    lo = nan_min(lo, x[i]);
                    hi = nan_max(hi, x[i]);
                }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, o, 64));
        hi = nan_max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        red[wave] = lo;
        red[4 + wave] = hi;
    }
    __syncthreads();
    lo = nan_min(nan_min(red[0], red[1]), nan_min(red[2], red[3]));
    hi = nan_max(nan_max(red[4], red[5]), nan_max(red[6], red[7]));
    const double span = hi - lo;

    // ---- pass 2: the plan's rows, t < 512
    const int t0 = 8 * lane;
    const int nv = n - t0 < 8 ? (n - t0 < 0 ? 0 : n - t0) : 8;
    for (int r = wave; r < rows; r += 4) {
        const int lead = (int)pl[3 + r];
        out_row = r < a.V ? a.data + ((int64_t)b * a.V + r) * BL : r == a.V ? a.target_view + (int64_t)b * BL
                                                                             : a.rest_view + ((int64_t)b * a.R + (r - a.V - 1)) * BL;
        double s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = 0.0;
        if (nv > 0) {
            if (lead < 8) {
                const int64_t e = off + (int64_t)lead * stride;
                load8(sig + e + t0, nv, elem_align<T>(e), s);
            } else {
                double x[8], y[8];
                load8(sig + off + t0, nv, elem_align<T>(off), x);
                load8(sig + off + stride + t0, nv, elem_align<T>(off + stride), y);
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = derived(lead - 8, x[i], y[i]);
            }
        }
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = i < nv ? (float)((s[i] - lo) / span) : 0.0f;
        reinterpret_cast<f32x4*>(out_row + t0)[0] = f32x4{v[0], v[1], v[2], v[3]};
        reinterpret_cast<f32x4*>(out_row + t0)[1] = f32x4{v[4], v[5], v[6], v[7]};
    }
}

}  // namespace

extern "C" {

size_t nef_beat_batch_args_bytes(void) { return sizeof(nef_beat_batch_args); }

int nef_beat_batch(const nef_beat_batch_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->signal && a->plan && a->data && a->target_view, NEF_E_NULL);
    NEF_REQUIRE(a->R == 0 || a->rest_view, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->V >= 1 && a->V <= 12 && a->R >= 0 && a->R <= 64, NEF_E_SHAPE);
    NEF_REQUIRE((a->dtype == 0 || a->dtype == 1) && a->signal_elems >= 1 && a->signal_elems < (1ll << 56), NEF_E_SHAPE);
    const uintptr_t bits = (uintptr_t)a->signal | (uintptr_t)a->data | (uintptr_t)a->target_view | (uintptr_t)a->rest_view;
    NEF_REQUIRE((bits & 15) == 0 && ((uintptr_t)a->plan & 7) == 0, NEF_E_UNSUPPORTED);
    if (a->dtype == 0)
        hipLaunchKernelGGL(beat_batch_kernel<int16_t>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(beat_batch_kernel<float>, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
