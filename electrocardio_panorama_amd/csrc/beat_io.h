// What the kernels that read device-resident recordings share (beats.hip: nef_beat_batch; recording.hip: nef_beat_range, nef_beat_stitch,
// nef_recording_stats): eight positions of a stored row as fp64 through the widest loads the row's address allows, numpy's NaN-keeping
// min / max, and the four derived limb leads as the host writes them; the check of a plan row and the lo / hi pass
// over a beat, which nef_beat_batch and nef_beat_range must form alike.
#pragma once

namespace {

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

// a plan row [offset of lead 0 at p_on, lead stride, n, `rows` leads] that stays inside a signal of signal_elems elements and names leads 0..11
__device__ __forceinline__ bool beat_row_ok(const int64_t* __restrict__ pl, int rows, int64_t signal_elems) {
    const int64_t off = pl[0], stride = pl[1], n64 = pl[2];
    bool ok = off >= 0 && off < signal_elems && stride >= 1 && stride <= signal_elems && n64 >= 1 && n64 <= stride &&
              n64 <= 0x7FFFFFF0ll && off + 7 * stride + n64 <= signal_elems;
    for (int r = 0; r < rows; ++r) ok = ok && pl[3 + r] >= 0 && pl[3 + r] < 12;
    return ok;
}

// lo / hi of one beat over 12 leads x n positions in fp64, by a 256-thread workgroup (every thread calls, every thread gets both): work
// items are (lead unit, group of 8 positions); unit 0 reads leads I and II and also forms the four derived leads, units 1..6 read one stored
// lead each.  `red` holds 8 doubles of LDS.
template <typename T>
__device__ __forceinline__ void beat_lo_hi(const T* __restrict__ sig, int64_t off, int64_t stride, int n, double* red, double& lo, double& hi) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int groups = (n + 7) >> 3;            // <= 2^28: 7 * groups fits an int
    lo = __builtin_inf(), hi = -__builtin_inf();
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
}

}  // namespace
