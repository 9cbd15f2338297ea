// Sliding median over lead-major rows of a device buffer (clean.py, dataset/resident.py: DATA.baseline_ms): the baseline
// estimate of a recording, or the recording minus it.  Definition: include/nefnet_hip.h (nef_sliding_median_args).
//
// nef_sliding_median   one workgroup per (table row, signal, tile of 1024 outputs).  The tile and its h positions of halo on each side
//                      (indices clamped to the row: edge replication) are staged in LDS once as order-preserving 32-bit keys -- -0.0 folded
//                      onto +0.0, a NaN as the largest key and counted -- beside their positions in the stretch; a thread takes groups of 8
//                      through load8.  The (key, position) pairs are then sorted by key in LDS (bitonic, padded to a power of two with
//                      pairs no window holds).  Each thread owns four outputs, lane + 256 j, and walks the sorted positions once for all
//                      four: every lane reads the same 16 bytes (an LDS broadcast) and counts, per output, the positions that lie in its
//                      window; per 32 pairs it notes the last chunk in front of which the count was still below h + 1.  A second, short
//                      walk over that one chunk finds the pair at which the count reaches h + 1: its key is the median.  A tile that
//                      staged a NaN also walks the tail of the sorted list, where the NaNs lie, and turns the outputs whose window holds
//                      one into NaN.
//
// The selected element is a stored value, so the result does not depend on the order of equal keys, on the tile cut or on the row's
// neighbours.  The kernel does not trust the table: a row that leaves a buffer writes nothing.  No state, no atomics, no scratch, one
// writer per element; an fp32 minuend may be dst itself (the thread that writes an element is the one that read it).
#include "nef_common.h"
#include "beat_io.h"

namespace {

constexpr int TILE = NEF_MEDIAN_TILE;
constexpr int MAX_H = NEF_MEDIAN_MAX_H;
constexpr int SORT_MAX = 2048;                  // pairs in LDS: 8 + 8 KiB
constexpr int CHUNK = 32;                       // pairs between two notes of the count
constexpr unsigned KEY_NAN = 0xFFFFFFFFu;       // above +inf's key (0xFF800000)
constexpr unsigned POS_NONE = 0x40000000u;      // a padding pair's position: in no window
static_assert(TILE == 4 * 256, "a thread owns 4 outputs of a tile");
static_assert(TILE + 2 * MAX_H <= SORT_MAX, "a tile and both halos fit the sort");
static_assert(SORT_MAX % CHUNK == 0 && CHUNK % 4 == 0, "the walk reads 4 positions at a time");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// a table row (offset, len, rows) that stays inside every buffer and inside the launch's extents
__device__ __forceinline__ bool median_row_ok(const int64_t* __restrict__ row, const nef_sliding_median_args& a) {
    const int64_t off = row[0], len = row[1], rows = row[2];
    if (!(len >= 1 && len <= a.max_len && rows >= 1 && rows <= a.max_rows && off >= 0)) return false;
    int64_t elems = a.src_elems < a.dst_elems ? a.src_elems : a.dst_elems;
    if (a.minuend && a.minuend_elems < elems) elems = a.minuend_elems;
    return len <= elems / rows && off <= elems - rows * len;
}

__device__ __forceinline__ unsigned median_key(float f, int& nans) {
    if (f != f) {
        ++nans;
        return KEY_NAN;
    }
    const unsigned u = f == 0.0f ? 0u : __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float median_value(unsigned k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

template <typename T>
__global__ __launch_bounds__(256) void sliding_median_kernel(const nef_sliding_median_args a) {
    __shared__ __attribute__((aligned(16))) unsigned key_s[SORT_MAX];
    __shared__ __attribute__((aligned(16))) unsigned pos_s[SORT_MAX];
    __shared__ int nan_s[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* __restrict__ row = a.table + 3 * (int64_t)blockIdx.z;
    if (!median_row_ok(row, a)) return;                                                 // block-uniform
    const int lead = (int)blockIdx.y;
    if (lead >= row[2]) return;                                                         // block-uniform
    const int64_t len64 = row[1];
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= len64) return;                                                            // block-uniform
    const int len = (int)len64, h = a.h;
    const int n_out = len64 - t0 < TILE ? (int)(len64 - t0) : TILE;                     // outputs of this tile
    const int n = n_out + 2 * h;                                                        // staged positions: t0 - h + [0, n)
    const int64_t base = row[0] + (int64_t)lead * len;
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.src) + base;

    int P = CHUNK;                                                                      // the sort's size: a power of two >= max(n, CHUNK)
    while (P < n) P <<= 1;

    // ---- x[clamp(t0 - h + r)] for r in [0, n) as keys, a group of 8 positions a thread; padding behind them
    int nans = 0;
    const int64_t b = t0 - h;
    for (int g = tid; 8 * g < P; g += 256) {
        const int64_t u0 = b + 8 * g;
        double x[8];
        if (8 * g + 8 <= n && u0 >= 0 && u0 + 8 <= len) {
            load8(sig + u0, 8, elem_align<T>(base + u0), x);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t q = u0 + i;
                x[i] = 8 * g + i < n ? (double)sig[q < 0 ? 0 : (q > len - 1 ? len - 1 : q)] : 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = 8 * g + i;
            if (r < n) {
                key_s[r] = median_key((float)x[i], nans);                               // exact: x came from an int16 or a float
                pos_s[r] = (unsigned)r;
            } else {
                key_s[r] = KEY_NAN;
                pos_s[r] = POS_NONE;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nans += __shfl_xor(nans, o, 64);
    if (lane == 0) nan_s[wave] = nans;
    __syncthreads();
    nans = nan_s[0] + nan_s[1] + nan_s[2] + nan_s[3];                                   // of the whole stretch, block-uniform

    // ---- sort the P pairs by key
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < (P >> 1); q += 256) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const int m = i | j;
                const unsigned ka = key_s[i], kb = key_s[m];
                if ((ka > kb) == ((i & k) == 0)) {
                    const unsigned pa = pos_s[i], pb = pos_s[m];
                    key_s[i] = kb, key_s[m] = ka;
                    pos_s[i] = pb, pos_s[m] = pa;
                }
            }
            __syncthreads();
        }
    }

    // ---- the four outputs lane + 256 j: output l's window is the positions [l, l + 2 h] of the stretch
    const unsigned w = 2u * (unsigned)h, need = (unsigned)h + 1u;
    unsigned lo[4], cnt[4], chunk[4], before[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = tid + 256 * j;
        lo[j] = l < n_out ? (unsigned)l : 0u;                                           // an output this tile lacks follows output 0, unstored
        cnt[j] = 0, chunk[j] = 0, before[j] = 0;
    }
    const int chunks = (n + CHUNK - 1) / CHUNK;                                         // <= P / CHUNK
    for (int c = 0; c < chunks; ++c) {
        bool open = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool below = cnt[j] < need;
            chunk[j] = below ? (unsigned)c : chunk[j];
            before[j] = below ? cnt[j] : before[j];
            open = open || below;
        }
        if (!__any(open)) break;                                                        // wave-uniform; no barrier below
        const u32x4* __restrict__ pp = reinterpret_cast<const u32x4*>(pos_s + CHUNK * c);
#pragma unroll
        for (int e = 0; e < CHUNK / 4; ++e) {
            const u32x4 p = pp[e];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cnt[j] += (p[i] - lo[j] <= w) ? 1u : 0u;
        }
    }

    const bool sub = a.minuend != nullptr;
    float* __restrict__ dst = a.dst + base + t0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = tid + 256 * j;
        // the pair of chunk[j] at which the count reaches h + 1
        unsigned c2 = before[j], at = CHUNK * chunk[j];
        const unsigned first = CHUNK * chunk[j];
        bool found = false;
        for (int e = 0; e < CHUNK; ++e) {
            const unsigned p = pos_s[first + (unsigned)e];
            c2 += (p - lo[j] <= w) ? 1u : 0u;
            const bool hit = !found && c2 == need;
            at = hit ? first + (unsigned)e : at;
            found = found || hit;
        }
        float m = median_value(key_s[at]);
        if (nans) {                                                                     // block-uniform: the NaNs and the padding are the tail
            bool any = false;
            for (int i = n - nans; i < P; ++i) any = any || (pos_s[i] - lo[j] <= w);
            m = any ? __builtin_nanf("") : m;
        }
        if (l < n_out) {
            if (sub) {
                const double v = a.minuend_dtype == 0 ? (double)reinterpret_cast<const int16_t*>(a.minuend)[base + t0 + l]
                                                      : (double)reinterpret_cast<const float*>(a.minuend)[base + t0 + l];
                dst[l] = (float)(v - (double)m);
            } else {
                dst[l] = m;
            }
        }
    }
}

}  // namespace

extern "C" {

size_t nef_sliding_median_args_bytes(void) { return sizeof(nef_sliding_median_args); }

int nef_sliding_median(const nef_sliding_median_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->src && a->table && a->dst, NEF_E_NULL);
    NEF_REQUIRE(a->N >= 1 && a->N <= 65535 && a->max_rows >= 1 && a->max_rows <= 65535 && a->max_len >= 1 && a->max_len <= 0x7FFF0000ll,
                NEF_E_SHAPE);
    NEF_REQUIRE(a->h >= 0 && a->h <= MAX_H && (a->dtype == 0 || a->dtype == 1) && (a->minuend_dtype == 0 || a->minuend_dtype == 1), NEF_E_SHAPE);
    NEF_REQUIRE(a->src_elems >= 1 && a->src_elems < (1ll << 56) && a->dst_elems >= 1 && a->dst_elems < (1ll << 56) &&
                (!a->minuend || (a->minuend_elems >= 1 && a->minuend_elems < (1ll << 56))), NEF_E_SHAPE);
    NEF_REQUIRE(((uintptr_t)a->src & 15) == 0 && ((uintptr_t)a->table & 7) == 0 && ((uintptr_t)a->dst & 3) == 0 &&
                ((uintptr_t)a->minuend & (a->minuend_dtype == 0 ? 1 : 3)) == 0, NEF_E_UNSUPPORTED);
    const dim3 grid((unsigned)nef_cdiv(a->max_len, TILE), (unsigned)a->max_rows, (unsigned)a->N);
    if (a->dtype == 0)
        hipLaunchKernelGGL((sliding_median_kernel<int16_t>), grid, dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL((sliding_median_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
