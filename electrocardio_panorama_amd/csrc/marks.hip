// Marks for unannotated recordings (dataset/marks.py): the QRS detector over a device-resident store.  Definitions:
// include/nefnet_hip.h (nef_mark_envelope_args, nef_mark_peaks_args).
//
// nef_mark_envelope   env(t) = the sum over a window of 2 H + 1 positions of the selected leads' squared central differences, fp64 from the
//                     stored values.  One workgroup per (recording, tile of 1024 positions): the tile of e plus its H halo is staged in LDS
//                     once (a thread takes groups of 8 positions through load8), then every position sums its window in ascending order.
// nef_mark_peaks      one workgroup per recording over its env: the segment maxima (a wave per segment), their lower median by rank
//                     counting, then tiles of 1024 positions with an r halo in LDS -- a thread tests its 4 consecutive positions, a block-wide
//                     prefix scan places the tile's peaks behind those of the tiles before it.
//
// No kernel keeps state, uses an atomic or scratch; every output element has one writer.  -ffp-contract=off keeps the multiply and each add
// of the envelope separately rounded: on an fp32 store the order written here is the definition.
#include "nef_common.h"
#include "beat_io.h"

namespace {

constexpr int TILE = NEF_MARK_TILE;
constexpr int MAX_H = NEF_MARK_MAX_H;
constexpr int MAX_R = NEF_MARK_MAX_R;
constexpr int MAX_SEG = NEF_MARK_MAX_SEGMENTS;
static_assert(TILE == 4 * 256, "a thread of the peaks kernel owns 4 consecutive positions of a tile");

__device__ __forceinline__ bool finite_d(double x) { return x - x == 0.0; }

// a table row (offset in `signal`, len, offset in `env`) that stays inside both buffers and inside the launch's max_len
__device__ __forceinline__ bool mark_row_ok(const int64_t* __restrict__ row, int64_t signal_elems, int64_t env_elems, int64_t max_len, bool with_signal) {
    const int64_t off = row[0], len = row[1], eoff = row[2];
    bool ok = len >= 1 && len <= max_len && eoff >= 0 && len <= env_elems && eoff <= env_elems - len;
    if (with_signal) ok = ok && off >= 0 && len <= signal_elems / 8 && off <= signal_elems - 8 * len;
    return ok;
}

// ------------------------------------------------------------------------------------------------------------ nef_mark_envelope
template <typename T>
__global__ __launch_bounds__(256) void mark_envelope_kernel(const nef_mark_envelope_args a) {
    __shared__ double es[TILE + 2 * MAX_H];
    const int tid = (int)threadIdx.x;
    const int64_t* __restrict__ row = a.table + 3 * (int64_t)blockIdx.y;
    if (!mark_row_ok(row, a.signal_elems, a.env_elems, a.max_len, true)) return;       // block-uniform
    const int64_t off = row[0], eoff = row[2];
    const int len = (int)row[1], t0 = (int)blockIdx.x * TILE, D = a.D, H = a.H;
    if (t0 >= len) return;                                                              // block-uniform
    const T* __restrict__ sig = reinterpret_cast<const T*>(a.signal);

    // ---- e(u) for u in [t0 - H, t0 + TILE + H) that lie in the recording; a group is 8 consecutive positions
    const int u_lo = t0 - H, span = TILE + 2 * H, groups = (span + 7) >> 3;
    for (int g = tid; g < groups; g += 256) {
        const int u0 = u_lo + 8 * g;
        if (u0 >= len || u0 + 8 <= 0) continue;
        double e[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int hi0 = u0 + D, lo0 = u0 - D;
        const bool hi_in = hi0 >= 0 && hi0 <= len - 8, lo_in = lo0 >= 0 && lo0 <= len - 8;
        for (int c = 0; c < 8; ++c) {
            if (!((a.lead_bits >> c) & 1)) continue;
            const int64_t base = off + (int64_t)c * len;
            double xh[8], xl[8];
            if (hi_in) {
                load8(sig + base + hi0, 8, elem_align<T>(base + hi0), xh);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = hi0 + i;
                    xh[i] = (double)sig[base + (q < 0 ? 0 : (q > len - 1 ? len - 1 : q))];
                }
            }
            if (lo_in) {
                load8(sig + base + lo0, 8, elem_align<T>(base + lo0), xl);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int q = lo0 + i;
                    xl[i] = (double)sig[base + (q < 0 ? 0 : (q > len - 1 ? len - 1 : q))];
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double d = xh[i] - xl[i];
                e[i] = e[i] + d * d;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 8 * g + i;
            if (k < span) es[k] = e[i];             // positions outside the recording hold a clamped value no window reads
        }
    }
    __syncthreads();

    // ---- env(t): the window in ascending order
    double* __restrict__ env = a.env + eoff;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        const int t = t0 + tid + 256 * j;
        if (t >= len) break;
        const int w0 = t - H < 0 ? 0 : t - H, w1 = t + H > len - 1 ? len - 1 : t + H;
        double s = 0.0;
        for (int u = w0; u <= w1; ++u) s = s + es[u - u_lo];
        env[t] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------ nef_mark_peaks
__global__ __launch_bounds__(256) void mark_peaks_kernel(const nef_mark_peaks_args a) {
    __shared__ double segmax[MAX_SEG];
    __shared__ double win[TILE + 2 * MAX_R];
    __shared__ double level_s;
    __shared__ int bad_s;
    __shared__ int wave_tot[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, rec = (int)blockIdx.x;
    const int64_t* __restrict__ row = a.table + 3 * (int64_t)rec;
    int32_t* __restrict__ out = a.peaks + (int64_t)rec * a.max_peaks;
    const double qnan = __builtin_nan("");

    bool ok = mark_row_ok(row, 0, a.env_elems, a.max_len, false);                      // block-uniform
    const int len = ok ? (int)row[1] : 1;
    const int seg = a.seg, nseg = len / seg > 1 ? len / seg : 1;
    ok = ok && nseg <= MAX_SEG;
    const double* __restrict__ env = a.env + (ok ? row[2] : 0);

    if (tid == 0) bad_s = 0;
    __syncthreads();
    if (ok) {
        // ---- segment maxima: wave w takes segments w, w + 4, ...; every position belongs to one segment, so this pass sees a non-finite value
        bool bad = false;
        for (int s = wave; s < nseg; s += 4) {
            const int b = s * seg, e = s == nseg - 1 ? len : b + seg;
            double m = -__builtin_inf();
            for (int t = b + lane; t < e; t += 64) {
                const double v = env[t];
                bad = bad || !finite_d(v);
                m = v > m ? v : m;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double w = __shfl_xor(m, o, 64);
                m = w > m ? w : m;
            }
            if (lane == 0) segmax[s] = m;
        }
        if (bad) bad_s = 1;                         // every writer stores the same word
    }
    __syncthreads();
    if (!ok || bad_s) {
        for (int k = tid; k < a.max_peaks; k += 256) out[k] = -1;
        if (tid == 0) {
            a.count[rec] = -1;
            a.level[rec] = qnan;
        }
        return;
    }

    // ---- the lower median: the value v with #(< v) <= rank < #(<= v); every thread that finds it stores the same word
    const int rank = (nseg - 1) / 2;
    for (int i = tid; i < nseg; i += 256) {
        const double v = segmax[i];
        int less = 0, le = 0;
        for (int j = 0; j < nseg; ++j) {
            const double w = segmax[j];
            less += w < v;
            le += w <= v;
        }
        if (less <= rank && rank < le) level_s = v;
    }
    __syncthreads();
    const double level = level_s, thr = level * a.frac;
    const int r = a.r;

    // ---- candidates, tile by tile
    int base = 0;
    for (int t0 = 0; t0 < len; t0 += TILE) {
        const int u_lo = t0 - r, span = TILE + 2 * r;
        __syncthreads();                            // the tile before is done with win and wave_tot
        for (int k = tid; k < span; k += 256) {
            const int u = u_lo + k;
            win[k] = (u >= 0 && u < len) ? env[u] : 0.0;
        }
        __syncthreads();
        int hit[4], c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + 4 * tid + j;
            bool pk = false;
            if (t < len) {
                const double v = win[t - u_lo];
                pk = v > 0.0 && v >= thr;
                if (pk) {
                    const int w0 = t - r < 0 ? 0 : t - r, w1 = t + r > len - 1 ? len - 1 : t + r;
                    for (int u = w0; u < t && pk; ++u) pk = win[u - u_lo] < v;
                    for (int u = t + 1; u <= w1 && pk; ++u) pk = win[u - u_lo] <= v;
                }
            }
            hit[j] = pk;
            c += pk;
        }
        // exclusive scan of c over the block: within the wave by shuffles, the waves in order
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int w = __shfl_up(incl, o, 64);
            if (lane >= o) incl += w;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = base + incl - c;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (hit[j]) {
                if (before < a.max_peaks) out[before] = t0 + 4 * tid + j;
                ++before;
            }
        base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    }
    for (int k = (base < a.max_peaks ? base : a.max_peaks) + tid; k < a.max_peaks; k += 256) out[k] = -1;
    if (tid == 0) {
        a.count[rec] = base;
        a.level[rec] = level;
    }
}

}  // namespace

extern "C" {

size_t nef_mark_envelope_args_bytes(void) { return sizeof(nef_mark_envelope_args); }
size_t nef_mark_peaks_args_bytes(void) { return sizeof(nef_mark_peaks_args); }

int nef_mark_envelope(const nef_mark_envelope_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->signal && a->table && a->env, NEF_E_NULL);
    NEF_REQUIRE(a->N >= 1 && a->N <= 65535 && a->max_len >= 1 && a->max_len <= 0x7FFF0000ll, NEF_E_SHAPE);
    NEF_REQUIRE(a->D >= 0 && a->D <= NEF_MARK_MAX_D && a->H >= 0 && a->H <= MAX_H && a->lead_bits >= 1 && a->lead_bits <= 255, NEF_E_SHAPE);
    NEF_REQUIRE((a->dtype == 0 || a->dtype == 1) && a->signal_elems >= 1 && a->signal_elems < (1ll << 56) && a->env_elems >= 1 &&
                a->env_elems < (1ll << 56), NEF_E_SHAPE);
    NEF_REQUIRE(((uintptr_t)a->signal & 15) == 0 && (((uintptr_t)a->table | (uintptr_t)a->env) & 7) == 0, NEF_E_UNSUPPORTED);
    const dim3 grid((unsigned)nef_cdiv(a->max_len, TILE), (unsigned)a->N);
    if (a->dtype == 0)
        hipLaunchKernelGGL(mark_envelope_kernel<int16_t>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(mark_envelope_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

int nef_mark_peaks(const nef_mark_peaks_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->env && a->table && a->peaks && a->count && a->level, NEF_E_NULL);
    NEF_REQUIRE(a->N >= 1 && a->max_len >= 1 && a->max_len <= 0x7FFF0000ll && a->env_elems >= 1 && a->env_elems < (1ll << 56), NEF_E_SHAPE);
    NEF_REQUIRE(a->seg >= 1 && a->max_len / a->seg <= MAX_SEG && a->r >= 0 && a->r <= MAX_R && a->max_peaks >= 1 && a->max_peaks <= (1 << 20), NEF_E_SHAPE);
    NEF_REQUIRE(a->frac == a->frac && a->frac >= 0.0 && a->frac - a->frac == 0.0, NEF_E_SHAPE);
    NEF_REQUIRE((((uintptr_t)a->env | (uintptr_t)a->table | (uintptr_t)a->level) & 7) == 0 && (((uintptr_t)a->peaks | (uintptr_t)a->count) & 3) == 0,
                NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(mark_peaks_kernel, dim3((unsigned)a->N), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
