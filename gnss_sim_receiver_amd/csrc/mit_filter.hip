// mit_filter.hip — interference mitigation for gfx950: pulse blanking and the two notch filters, the
// Signal_Conditioner's other InputFilter choices.
//
// Replaces src/algorithms/input_filter/gnuradio_blocks/pulse_blanking_cc.cc:57-98, notch_cc.cc:63-121 and
// notch_lite_cc.cc:71-138 (adapters: input_filter/adapters/{pulse_blanking_filter,notch_filter,
// notch_filter_lite}.cc).  The blocks' `while ((index + length_) < noutput_items)` loops depend on the
// scheduler only in when a segment is emitted; here each block is defined on the stream: segments of
// `length` samples from the first sample, through the state machine in order, a run emits every complete
// segment and keeps the rest and all state on the device.
//
// The notch keeps the block's one-sample advance: notch_cc.cc:72 does `in++` without a history, so output
// sample k is formed from input sample k + 1 with input sample k as the "previous" one, and segment s is
// complete once input sample (s + 1)·length has arrived.  The lite form has set_history(2): output k from
// input k, previous k − 1, zero before the stream.
//
// Per run, over V = carry ‖ in (carry[0] = the sample before the first unemitted output position, then the
// pending samples), cur(j) = V[off + j] the block's in[j], off = 1 (pulse blanking, lite) or 2 (notch):
//   mit_stats_kernel   lane s forms segment s's energy as the serial float sum of re·re + im·im (the
//                      accumulator of volk_32f_accumulator_s32f / the real part of VOLK's generic
//                      conjugate dot product) and, lite, the z0 the segment would set (:104-112).
//   mit_scan_kernel    one workgroup walks the segment state machine in order out of LDS tiles of the
//                      energies; a tile that cannot hold an estimation segment is decided by all lanes at
//                      once (the lite form's z0 in force from a scan of the run starts), any other is
//                      walked by one lane; an estimation segment of a notch (direct DFT with twiddles rounded once from double,
//                      power spectrum, noise floor) is worked by the whole workgroup.  Writes
//                      a code per segment (0 copy, 1 filter, 2 filter after clearing last_out), lite's z0
//                      per segment, the carried state and the next run's carry.
//   mit_apply_kernel   lane j: copy / zero, or a[j] = p_c·z0, b[j] = x − z0·prev for the chain.
//   chain              y[j] = b[j] + a[j]·y[j − 1], serial by definition:
//     mit_chain_serial_kernel  the lane of a run's first segment runs the whole maximal run of filtered
//                      segments (runs start from last_out = 0, so they are independent);
//     mit_chain_spec_kernel + mit_chain_fix_kernel  lane c runs chunk c of chunk_segs segments; where its
//                      first segment continues a run it first walks warm_segs segments ahead of it from the
//                      zero state without writing (exact, not a prediction, if that walk meets the run's
//                      start or the run's first segment).  Since |a| = p_c < 1 a chain from a wrong state
//                      becomes bitwise equal to the true one after a bounded number of samples and stays
//                      equal.  The fix kernel compares each predicted start state bitwise with the
//                      predecessor's final state in chunk order and replays refuted chunks serially.
// Everything in the chain, a, b, the energies and the state machine is float arithmetic of defined order
// with contraction off: bit-exact against tests/mit_model.py.
#include <cmath>
#include <cstring>
#include <new>

#include "host_api.h"
#include "glibc_atanf.h"
#include "glibc_sincosf.h"

#pragma clang fp contract(off)

using namespace gnsship;

namespace {

constexpr int kMitThreads = 256;
constexpr int kMitMaxLen = GNSSHIP_MIT_MAX_LENGTH;
constexpr int kMitScanTile = 1024;     // energies per LDS tile of the scan
constexpr int kMitChunkTarget = 2048;  // samples per speculative chunk, at least
constexpr int kMitWarmupCap = 4096;    // warm-up samples, at most (p_c_factor near or above 1)

// The carried members of the block.
struct MitDevState {
    float noise;
    int32_t n_segments;
    int32_t flag;     // last_filtered_ / filter_state_
    int32_t n_coeff;  // n_segments_coeff_
    float2 z0;
    float2 last[2];   // last_out_, double-buffered: a run reads [cur], writes [cur ^ 1]
    unsigned long long speculated, replayed;
};

struct MitArgs {
    const float2* in;
    const float2* carry_old;  // [0] history sample, [1 .. n_carry) pending
    float2* carry_new;
    float2* out;
    float2* a;        // chain coefficients (notches)
    float2* b;
    float* energy;    // per segment
    float2* zseg;     // lite: z0 in force in segment s / stats: the z0 segment s would set
    uint8_t* code;    // per segment
    float2* y_pred;   // per chunk
    float2* y_end;
    uint8_t* spec;
    MitDevState* st;
    const float2* twiddle;  // e^{−j2πm/L}, m < L
    int64_t n_in;
    int32_t n_carry;      // 1 + pending
    int32_t n_carry_new;
    int32_t nseg;
    int32_t len;
    int32_t kind;
    int32_t off;          // cur(j) = V[off + j]
    int32_t n_est, n_reset, n_coeff_reset;
    int32_t cur;          // which last[] is current
    int32_t chunk_segs, warm_segs, nchunks;
    float thres, p_c;
};

__device__ __forceinline__ float2 mit_v(const MitArgs& a, int64_t i)
{
    return i < a.n_carry ? a.carry_old[i] : a.in[i - a.n_carry];
}

// std::complex<float> product as libgcc's __mulsc3 forms it for finite values: (ac − bd, ad + bc).
__device__ __forceinline__ float2 mit_cmul(float2 x, float2 y)
{
    return make_float2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x);
}

// z0 = std::exp(gr_complex(0, 1)·angle) as glibc's cexpf evaluates it: (cosf, sinf); |angle| <= FLT_MIN
// takes its (1, angle) branch, which is what sincosf returns there too.
__device__ __forceinline__ float2 mit_z0(float angle)
{
    float s, c;
    glibc_sincosf(angle, &s, &c);
    return make_float2(c, s);
}

// volk_32fc_x2_multiply_conjugate_32fc + volk_32fc_s32f_atan2_32f (normalisation 1.0): atan2f of x·conj(p)
__device__ __forceinline__ float mit_angle(float2 x, float2 p)
{
    const float2 c = mit_cmul(x, make_float2(p.x, -p.y));
    return glibc_atan2f(c.y, c.x);
}

__global__ __launch_bounds__(kMitThreads) void mit_stats_kernel(const MitArgs a)
{
    const int s = blockIdx.x * kMitThreads + threadIdx.x;
    if (s >= a.nseg) return;
    const int64_t j0 = static_cast<int64_t>(s) * a.len + a.off;
    float e = 0.0f;
    for (int i = 0; i < a.len; i++) {
        const float2 x = mit_v(a, j0 + i);
        e = e + (x.x * x.x + x.y * x.y);
    }
    a.energy[s] = e;
    if (a.kind == GNSSHIP_MIT_NOTCH_LITE) {
        // notch_lite_cc.cc:106-111
        const float angle1 = mit_angle(mit_v(a, j0 + 1), mit_v(a, j0));
        const float angle2 = mit_angle(mit_v(a, j0 + a.len - 1), mit_v(a, j0 + a.len - 2));
        a.zseg[s] = mit_z0((angle1 + angle2) / 2.0f);
    }
}

// One workgroup.  sh_x / sh_w / sh_p serve the notches' estimation segments.
__global__ __launch_bounds__(kMitThreads) void mit_scan_kernel(const MitArgs a)
{
    __shared__ float sh_e[kMitScanTile];
    __shared__ uint8_t sh_d[kMitScanTile];  // fast path: E/noise > thres
    __shared__ float sh_noise;
    __shared__ int sh_flag, sh_fast, sh_ncoeff, sh_ncoeff_out, sh_last;
    __shared__ float2 sh_z0, sh_z0_out;
    __shared__ int sh_rs[2][kMitScanTile];  // fast path, lite: run starts
    __shared__ float2 sh_x[kMitMaxLen];
    __shared__ float2 sh_w[kMitMaxLen];
    __shared__ float sh_p[kMitMaxLen];
    __shared__ int sh_stop;
    const int tid = threadIdx.x;
    const int L = a.len;
    const bool notch = a.kind != GNSSHIP_MIT_PULSE_BLANKING;

    // the next run's carry: V from the first position this run does not emit
    for (int i = tid; i < a.n_carry_new; i += kMitThreads) a.carry_new[i] = mit_v(a, static_cast<int64_t>(a.nseg) * L + i);
    if (a.nseg == 0) {
        if (tid == 0) a.st->last[a.cur ^ 1] = a.st->last[a.cur];
        return;
    }
    if (notch)
        for (int i = tid; i < L; i += kMitThreads) sh_w[i] = a.twiddle[i];

    // thread 0's copy of the members
    float noise = 0.0f;
    int n_segments = 0, flag = 0, n_coeff = 0;
    float2 z0 = make_float2(0.0f, 0.0f);
    if (tid == 0) {
        noise = a.st->noise;
        n_segments = a.st->n_segments;
        flag = a.st->flag;
        n_coeff = a.st->n_coeff;
        z0 = a.st->z0;
    }
    const float deg = static_cast<float>(2 * L);

    for (int base = 0; base < a.nseg; base += kMitScanTile) {
        const int tile_end = min(base + kMitScanTile, a.nseg);
        // Fast path: a tile that cannot hold an estimation segment (n_segments_ is past the window and stays there:
        // no reset can fall in the tile) is decided by all lanes at once — the segment's comparison, for the notches
        // whether its predecessor was filtered, and for the lite form the z0 in force: segment i of a run that
        // started at segment rs has n_segments_coeff_ = (i − rs) mod R on entry (c0 + i for the run carried into
        // the tile), and the z0 of the last segment where that was 0.
        const int len = tile_end - base;
        if (tid == 0) {
            sh_noise = noise;
            sh_flag = flag;
            sh_ncoeff = n_coeff;
            sh_z0 = z0;
            sh_last = -1;
            sh_fast = n_segments >= a.n_est && n_segments <= a.n_reset - len;
        }
        __syncthreads();
        const bool fast = sh_fast != 0;
        const float noise_tile = sh_noise;
        for (int i = base + tid; i < tile_end; i += kMitThreads) {
            const float e = a.energy[i];
            sh_e[i - base] = e;
            if (fast) sh_d[i - base] = e / noise_tile > a.thres ? 1 : 0;
        }
        __syncthreads();
        if (fast) {
            for (int i = tid; i < len; i += kMitThreads) {
                const int prev = i ? sh_d[i - 1] : sh_flag;
                a.code[base + i] = sh_d[i] ? (notch ? (prev ? 1 : 2) : 1) : 0;
            }
            if (a.kind == GNSSHIP_MIT_NOTCH_LITE) {
                // run starts by a max-scan of the start markers (−1: the run carried into the tile, or none)
                for (int i = tid; i < len; i += kMitThreads) {
                    const int prev = i ? sh_d[i - 1] : sh_flag;
                    sh_rs[0][i] = sh_d[i] && !prev ? i : -1;
                    if (sh_d[i]) atomicMax(&sh_last, i);
                }
                __syncthreads();
                int cur = 0;
                for (int off = 1; off < len; off <<= 1) {
                    for (int i = tid; i < len; i += kMitThreads) {
                        int v = sh_rs[cur][i];
                        if (i >= off) v = max(v, sh_rs[cur][i - off]);
                        sh_rs[cur ^ 1][i] = v;
                    }
                    __syncthreads();
                    cur ^= 1;
                }
                const int R = a.n_coeff_reset, c0 = sh_ncoeff;
                const int last = sh_last;
                for (int i = tid; i < len; i += kMitThreads) {
                    if (!sh_d[i]) continue;
                    const int rs = sh_rs[cur][i];
                    const int k = rs >= 0 ? (i - rs) % R : (c0 + i) % R;
                    const int leader = i - k;  // >= rs, or before the tile in the carried run
                    const float2 z = leader >= 0 ? a.zseg[base + leader] : sh_z0;
                    if (k != 0) a.zseg[base + i] = z;  // a leader already holds its own
                    if (i == last) {
                        sh_ncoeff_out = (k + 1) % R;
                        sh_z0_out = z;
                    }
                }
                __syncthreads();
                if (tid == 0 && last >= 0) {
                    n_coeff = sh_ncoeff_out;
                    z0 = sh_z0_out;
                }
            }
            if (tid == 0) {
                flag = sh_d[len - 1];
                n_segments += len;
            }
            continue;  // the barrier at the top of the next tile orders the reuse of the shared arrays
        }
        int pos = base;
        while (true) {
            if (tid == 0) {
                int s = pos;
                for (; s < tile_end; s++) {
                    const float e = sh_e[s - base];
                    if (n_segments < a.n_est && flag == 0) {
                        if (notch) break;  // the workgroup estimates
                        noise = (static_cast<float>(n_segments) * noise + e / deg) / static_cast<float>(n_segments + 1);
                        a.code[s] = 0;
                    } else if (e / noise > a.thres) {
                        if (notch) {
                            a.code[s] = flag ? 1 : 2;
                            if (!flag) n_coeff = 0;
                            if (a.kind == GNSSHIP_MIT_NOTCH_LITE) {
                                if (n_coeff == 0) z0 = a.zseg[s];
                                a.zseg[s] = z0;
                                n_coeff = (n_coeff + 1) % a.n_coeff_reset;
                            }
                        } else {
                            a.code[s] = 1;
                        }
                        flag = 1;
                    } else {
                        a.code[s] = 0;
                        flag = 0;
                        if (n_segments > a.n_reset) n_segments = 0;
                    }
                    n_segments++;
                }
                sh_stop = s;
            }
            __syncthreads();
            const int s = sh_stop;
            if (s >= tile_end) break;
            // estimation segment s of a notch: |DFT|² in dB, noise floor, linear (notch_cc.cc:77-82)
            const int64_t j0 = static_cast<int64_t>(s) * L + a.off;
            for (int i = tid; i < L; i += kMitThreads) sh_x[i] = mit_v(a, j0 + i);
            __syncthreads();
            for (int k = tid; k < L; k += kMitThreads) {
                float re = 0.0f, im = 0.0f;
                int m = 0;
                for (int n = 0; n < L; n++) {
                    const float2 x = sh_x[n], w = sh_w[m];
                    re = re + (x.x * w.x - x.y * w.y);
                    im = im + (x.x * w.y + x.y * w.x);
                    m += k;
                    if (m >= L) m -= L;
                }
                // volk_32fc_s32f_power_spectrum_32f, generic, normalisation 1.0: the 1e-20 is a double
                const float p = static_cast<float>(static_cast<double>(re * re + im * im) + 1e-20);
                sh_p[k] = 10.0f * log10f(p);
            }
            __syncthreads();
            if (tid == 0) {
                // volk_32f_s32f_calc_spectral_noise_floor_32f, generic, exclusion 15 dB
                float sum = 0.0f;
                for (int i = 0; i < L; i++) sum = sum + sh_p[i];
                const float mean = sum / static_cast<float>(L) + 15.0f;
                int cnt = L;
                for (int i = 0; i < L; i++)
                    if (sh_p[i] > mean) {
                        sum = sum - sh_p[i];
                        cnt--;
                    }
                const float db = cnt == 0 ? mean : sum / static_cast<float>(cnt);
                const float lin = powf(10.0f, db / 10.0f) / deg;
                noise = (static_cast<float>(n_segments) * noise + lin) / static_cast<float>(n_segments + 1);
                a.code[s] = 0;
                n_segments++;
            }
            pos = s + 1;
            __syncthreads();
        }
    }
    if (tid == 0) {
        a.st->noise = noise;
        a.st->n_segments = n_segments;
        a.st->flag = flag;
        a.st->n_coeff = n_coeff;
        a.st->z0 = z0;
        if (!notch) a.st->last[a.cur ^ 1] = a.st->last[a.cur];
    }
}

__global__ __launch_bounds__(kMitThreads) void mit_apply_kernel(const MitArgs a)
{
    const int64_t n_out = static_cast<int64_t>(a.nseg) * a.len;
    const float2 pc = make_float2(a.p_c, 0.0f);
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kMitThreads + threadIdx.x; j < n_out; j += static_cast<int64_t>(gridDim.x) * kMitThreads) {
        const int s = static_cast<int>(j / a.len);
        const int code = a.code[s];
        const float2 x = mit_v(a, j + a.off);
        if (code == 0) {
            a.out[j] = x;
        } else if (a.kind == GNSSHIP_MIT_PULSE_BLANKING) {
            a.out[j] = make_float2(0.0f, 0.0f);
        } else {
            const float2 p = mit_v(a, j + a.off - 1);
            const float2 z0 = a.kind == GNSSHIP_MIT_NOTCH ? mit_z0(mit_angle(x, p)) : a.zseg[s];
            const float2 zp = mit_cmul(z0, p);
            a.b[j] = make_float2(x.x - zp.x, x.y - zp.y);
            a.a[j] = mit_cmul(pc, z0);
        }
    }
}

// Segments [s_from, s_to) of the chain from state y: code 0 leaves y alone (the next filtered segment is a
// 2), 2 clears it, then out = b + a·y sample after sample.
template <bool kWrite>
__device__ __forceinline__ float2 mit_chain(const MitArgs& a, int s_from, int s_to, float2 y)
{
    for (int s = s_from; s < s_to; s++) {
        const int code = a.code[s];
        if (code == 0) continue;
        if (code == 2) y = make_float2(0.0f, 0.0f);
        const int64_t j0 = static_cast<int64_t>(s) * a.len;
        int i = 0;
        for (; i + 8 <= a.len; i += 8) {
            float2 ca[8], cb[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                ca[u] = a.a[j0 + i + u];
                cb[u] = a.b[j0 + i + u];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const float2 t = mit_cmul(ca[u], y);
                y = make_float2(cb[u].x + t.x, cb[u].y + t.y);
                if (kWrite) a.out[j0 + i + u] = y;
            }
        }
        for (; i < a.len; i++) {
            const float2 t = mit_cmul(a.a[j0 + i], y);
            const float2 bb = a.b[j0 + i];
            y = make_float2(bb.x + t.x, bb.y + t.y);
            if (kWrite) a.out[j0 + i] = y;
        }
    }
    return y;
}

__global__ __launch_bounds__(64) void mit_chain_serial_kernel(const MitArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.nseg) return;
    const int code = a.code[s];
    const bool start = code == 2 || (s == 0 && code == 1);
    if (start) {
        int e = s + 1;
        while (e < a.nseg && a.code[e] == 1) e++;
        const float2 y = mit_chain<true>(a, s, e, a.st->last[a.cur]);
        if (e == a.nseg) a.st->last[a.cur ^ 1] = y;
    } else if (code == 0 && s == a.nseg - 1) {
        a.st->last[a.cur ^ 1] = a.st->last[a.cur];
    }
}

__global__ __launch_bounds__(64) void mit_chain_spec_kernel(const MitArgs a)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.nchunks) return;
    const int s0 = c * a.chunk_segs, s1 = min(s0 + a.chunk_segs, a.nseg);
    float2 y = a.st->last[a.cur];
    int spec = 0;
    if (c > 0 && a.code[s0] == 1) {
        const int sb = max(s0 - a.warm_segs, 0);
        // exact when the walk starts at the run's carried state or meets the run's first segment
        bool exact = sb == 0;
        for (int s = sb; s < s0 && !exact; s++) exact = a.code[s] != 1;
        if (sb > 0) y = make_float2(0.0f, 0.0f);
        y = mit_chain<false>(a, sb, s0, y);
        spec = exact ? 0 : 1;
    }
    a.y_pred[c] = y;
    a.spec[c] = static_cast<uint8_t>(spec);
    a.y_end[c] = mit_chain<true>(a, s0, s1, y);
}

__global__ void mit_chain_fix_kernel(const MitArgs a)
{
    unsigned long long speculated = 0, replayed = 0;
    for (int c = 1; c < a.nchunks; c++) {
        if (!a.spec[c]) continue;
        speculated++;
        const float2 p = a.y_pred[c], t = a.y_end[c - 1];
        if (__float_as_uint(p.x) != __float_as_uint(t.x) || __float_as_uint(p.y) != __float_as_uint(t.y)) {
            replayed++;
            const int s0 = c * a.chunk_segs, s1 = min(s0 + a.chunk_segs, a.nseg);
            a.y_end[c] = mit_chain<true>(a, s0, s1, t);
        }
    }
    a.st->speculated += speculated;
    a.st->replayed += replayed;
    a.st->last[a.cur ^ 1] = a.code[a.nseg - 1] != 0 ? a.y_end[a.nchunks - 1] : a.st->last[a.cur];
}

// log Q(a, x) = −x + log Σ_{k<a} x^k/k! for integer a, its terms scaled by the last one (they overflow a
// double from a of a few hundred), and Newton on it: include/gnsship_cpp.hpp's gamma_p_inv_int restated
// for a up to 1024.  Returns the x with Q(a, x) = q.
double mit_gamma_q_inv_int(int a, double q)
{
    const double logq = std::log(q);
    double x = std::max(1.0, a - logq);
    for (int it = 0; it < 200; it++) {
        double term = 1.0, sum = 1.0;  // x^k/k! over x^{a−1}/(a−1)!, from k = a − 1 down
        for (int k = a - 1; k >= 1; k--) {
            term *= k / x;
            sum += term;
            if (term < 1e-300) break;
        }
        const double lq = -x + std::log(sum) + (a - 1) * std::log(x) - std::lgamma(static_cast<double>(a));
        const double dlq = -1.0 / sum;
        const double step = (lq - logq) / dlq;
        x -= step;
        if (!(x > 0.0)) x = 1e-12;
        if (std::fabs(step) < 1e-14 * std::max(1.0, x)) break;
    }
    return x;
}

}  // namespace

struct gnsship_mit {
    gnsship_ctx* ctx = nullptr;
    gnsship_mit_conf conf = {};
    float thres = 0.0f;
    int chain_form = GNSSHIP_MIT_CHAIN_SERIAL;
    int off = 1;
    int chunk_segs = 1, warm_segs = 1;
    int64_t max_in = 0, out_cap = 0;
    int64_t n_pending = 0;
    uint64_t samples_in = 0, samples_out = 0;
    int cur = 0, carry_cur = 0;
    float2* carry_dev[2] = {nullptr, nullptr};
    float2* out_dev = nullptr;
    float2* a_dev = nullptr;
    float2* b_dev = nullptr;
    float* energy_dev = nullptr;
    float2* zseg_dev = nullptr;
    uint8_t* code_dev = nullptr;
    float2* y_pred_dev = nullptr;
    float2* y_end_dev = nullptr;
    uint8_t* spec_dev = nullptr;
    MitDevState* st_dev = nullptr;
    float2* twiddle_dev = nullptr;
    DevBuf stage_dev;  // host input: sized once, to max_in samples, at the first host run
};

extern "C" int gnsship_mit_threshold(double pfa, int length, float* thres)
{
    if (!thres || !(pfa > 0.0) || !(pfa < 1.0) || length < 2 || length > kMitMaxLen) return GNSSHIP_E_INVAL;
    // chi²(2·length) upper quantile = 2·(x with Q(length, x) = pfa)
    const double x = 2.0 * mit_gamma_q_inv_int(length, pfa);
    if (!std::isfinite(x)) return GNSSHIP_E_INVAL;
    *thres = static_cast<float>(x);
    return GNSSHIP_OK;
}

extern "C" int gnsship_mit_destroy(gnsship_mit* m)
{
    if (!m) return GNSSHIP_E_INVAL;
    quiesce(m->ctx);
    free_all({m->carry_dev[0], m->carry_dev[1], m->out_dev, m->a_dev, m->b_dev, m->energy_dev, m->zseg_dev, m->code_dev, m->y_pred_dev,
        m->y_end_dev, m->spec_dev, m->st_dev, m->twiddle_dev});
    release(m->stage_dev);
    delete m;
    return GNSSHIP_OK;
}

extern "C" int gnsship_mit_reset(gnsship_mit* m)
{
    if (!m) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = m->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipError_t e = hipMemsetAsync(m->st_dev, 0, sizeof(MitDevState), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->carry_dev[m->carry_cur], 0, sizeof(float2), ctx->stream);  // zero history sample
    if (e != hipSuccess) return hip_fail(ctx, e, "gnsship_mit_reset");
    m->n_pending = 0;
    m->samples_in = m->samples_out = 0;
    return GNSSHIP_OK;
}

extern "C" int gnsship_mit_create(gnsship_ctx* ctx, const gnsship_mit_conf* conf, int64_t max_in_samples, gnsship_mit** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: null configuration");
    if (conf->kind < GNSSHIP_MIT_PULSE_BLANKING || conf->kind > GNSSHIP_MIT_NOTCH_LITE) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: unknown kind");
    if (conf->length < 2 || conf->length > kMitMaxLen) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: 2 <= length <= 1024");
    if (conf->n_segments_est < 1) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: n_segments_est >= 1");
    if (conf->kind == GNSSHIP_MIT_NOTCH_LITE && conf->n_segments_coeff < 1)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: n_segments_coeff >= 1");
    if (conf->chain_form < GNSSHIP_MIT_CHAIN_AUTO || conf->chain_form > GNSSHIP_MIT_CHAIN_SPECULATIVE)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: unknown chain form");
    if (max_in_samples < 1 || max_in_samples > GNSSHIP_MIT_MAX_IN_SAMPLES) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: 1 <= max_in_samples <= 2^30");
    float thres = conf->threshold;
    if (!(thres > 0.0f)) {
        if (!(conf->pfa > 0.0f) || !(conf->pfa < 1.0f) || gnsship_mit_threshold(conf->pfa, conf->length, &thres) != GNSSHIP_OK)
            return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_create: pfa must be in (0, 1) when no threshold is given");
    }
    if (int rc = set_device(ctx)) return rc;
    gnsship_mit* m = new (std::nothrow) gnsship_mit();
    if (!m) return GNSSHIP_E_NOMEM;
    m->ctx = ctx;
    m->conf = *conf;
    m->thres = thres;
    m->max_in = max_in_samples;
    const int L = conf->length;
    m->off = conf->kind == GNSSHIP_MIT_NOTCH ? 2 : 1;
    // Warm-up: a state error decays as p_c^n, below one float ulp of the state (2^-24) after
    // n0 = 24·ln2/−ln(p_c) samples; twice that plus a segment (the measured worst start needed 1.35·n0 at
    // p_c = 0.9, over 1.5·n0 at 0.99), in whole segments, capped where p_c is near or above 1.
    const double pc = std::fabs(static_cast<double>(conf->p_c_factor));
    int64_t warm = kMitWarmupCap;
    if (pc < 1.0) {
        const double n0 = pc > 0.0 ? std::ceil(24.0 * std::log(2.0) / -std::log(pc)) : 1.0;
        if (2.0 * n0 < kMitWarmupCap) warm = static_cast<int64_t>(2.0 * n0);
    }
    m->warm_segs = static_cast<int>((warm + L - 1) / L) + 1;
    m->chunk_segs = std::max((kMitChunkTarget + L - 1) / L, 4 * m->warm_segs);
    // AUTO: the speculative form wherever the warm-up is derived from p_c_factor and not the cap (DESIGN.md §8:
    // on one unbroken filtered run the serial form is a single lane, below real time at 50 Msps, the speculative
    // form over a hundred times faster; on short runs both are far above any stream rate); the serial form where
    // it is capped and speculation would be refuted.
    m->chain_form = conf->chain_form;
    if (m->chain_form == GNSSHIP_MIT_CHAIN_AUTO) m->chain_form = warm < kMitWarmupCap ? GNSSHIP_MIT_CHAIN_SPECULATIVE : GNSSHIP_MIT_CHAIN_SERIAL;
    m->out_cap = max_in_samples + L + 1;
    const int64_t seg_cap = m->out_cap / L + 1;
    const int64_t chunk_cap = seg_cap / m->chunk_segs + 1;
    const bool notch = conf->kind != GNSSHIP_MIT_PULSE_BLANKING;
    hipError_t e = alloc_all(ctx, {dev_alloc(&m->carry_dev[0], L + 2), dev_alloc(&m->carry_dev[1], L + 2), dev_alloc(&m->out_dev, m->out_cap),
                                      dev_alloc(&m->energy_dev, seg_cap), dev_alloc(&m->code_dev, seg_cap), dev_alloc(&m->st_dev, 1)});
    if (notch) {
        if (e == hipSuccess)
            e = alloc_all(ctx, {dev_alloc(&m->a_dev, m->out_cap), dev_alloc(&m->b_dev, m->out_cap), dev_alloc(&m->zseg_dev, seg_cap),
                                   dev_alloc(&m->y_pred_dev, chunk_cap), dev_alloc(&m->y_end_dev, chunk_cap), dev_alloc(&m->spec_dev, chunk_cap)});
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&m->twiddle_dev), sizeof(float2) * L);
        if (e == hipSuccess) {
            float2 tw[kMitMaxLen];
            const double pi = 3.14159265358979323846;
            for (int i = 0; i < L; i++) {
                const double ph = 2.0 * pi * static_cast<double>(i) / static_cast<double>(L);
                tw[i] = make_float2(static_cast<float>(std::cos(ph)), static_cast<float>(-std::sin(ph)));
            }
            e = hipMemcpy(m->twiddle_dev, tw, sizeof(float2) * L, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        gnsship_mit_destroy(m);
        return hip_fail(ctx, e, "gnsship_mit_create");
    }
    if (int rc = gnsship_mit_reset(m)) {
        gnsship_mit_destroy(m);
        return rc;
    }
    *out = m;
    return GNSSHIP_OK;
}

extern "C" int gnsship_mit_state_get(gnsship_mit* m, gnsship_mit_state* st)
{
    if (!m || !st) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = m->ctx;
    if (int rc = set_device(ctx)) return rc;
    MitDevState d;
    if (int rc = copy_out(ctx, {{&d, m->st_dev, sizeof(d)}}, "gnsship_mit_state_get")) return rc;
    st->noise_power = d.noise;
    st->threshold = m->thres;
    st->n_segments = d.n_segments;
    st->n_segments_coeff = d.n_coeff;
    st->filter_state = d.flag;
    st->chain_form = m->chain_form;
    st->samples_in = m->samples_in;
    st->samples_out = m->samples_out;
    st->pending_samples = m->n_pending;
    st->chunk_samples = static_cast<int64_t>(m->chunk_segs) * m->conf.length;
    st->warmup_samples = static_cast<int64_t>(m->warm_segs) * m->conf.length;
    st->chunks_speculated = d.speculated;
    st->chunks_replayed = d.replayed;
    return GNSSHIP_OK;
}

extern "C" int gnsship_mit_run(gnsship_mit* m, const void* in, int in_on_device, int64_t n_in, void* dev_dst, float* host_out,
    void** dev_out, int64_t* n_out)
{
    if (!m) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = m->ctx;
    if (n_in < 0 || n_in > m->max_in) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_run: 0 <= n_in <= max_in_samples");
    if (n_in > 0 && !in) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_mit_run: null input");
    if (int rc = set_device(ctx)) return rc;
    const void* src = in;
    if (!in_on_device && n_in > 0) {
        // sized once, at the first host run, to the largest run there can be
        if (int rc = stage(ctx, m->stage_dev, in, sizeof(float2) * static_cast<size_t>(n_in), "gnsship_mit_run", "stage",
                sizeof(float2) * static_cast<size_t>(m->max_in)))
            return rc;
        src = m->stage_dev.dev;
    }
    const int L = m->conf.length;
    const int64_t avail = m->n_pending + n_in;  // <= max_in + L
    // the notch reads one sample past the segment (its one-sample advance)
    const int64_t nseg = m->off == 2 ? (avail >= 1 ? (avail - 1) / L : 0) : avail / L;
    MitArgs a = {};
    a.in = static_cast<const float2*>(src);
    a.carry_old = m->carry_dev[m->carry_cur];
    a.carry_new = m->carry_dev[m->carry_cur ^ 1];
    a.out = dev_dst ? static_cast<float2*>(dev_dst) : m->out_dev;
    a.a = m->a_dev;
    a.b = m->b_dev;
    a.energy = m->energy_dev;
    a.zseg = m->zseg_dev;
    a.code = m->code_dev;
    a.y_pred = m->y_pred_dev;
    a.y_end = m->y_end_dev;
    a.spec = m->spec_dev;
    a.st = m->st_dev;
    a.twiddle = m->twiddle_dev;
    a.n_in = n_in;
    a.n_carry = static_cast<int32_t>(1 + m->n_pending);
    a.n_carry_new = static_cast<int32_t>(1 + avail - nseg * L);  // <= L + 2
    a.nseg = static_cast<int32_t>(nseg);
    a.len = L;
    a.kind = m->conf.kind;
    a.off = m->off;
    a.n_est = m->conf.n_segments_est;
    a.n_reset = m->conf.n_segments_reset;
    a.n_coeff_reset = m->conf.n_segments_coeff;
    a.cur = m->cur;
    a.chunk_segs = m->chunk_segs;
    a.warm_segs = m->warm_segs;
    a.nchunks = static_cast<int32_t>((nseg + m->chunk_segs - 1) / m->chunk_segs);
    a.thres = m->thres;
    a.p_c = m->conf.p_c_factor;
    const int64_t nk = nseg * L;
    if (nseg > 0) hipLaunchKernelGGL(mit_stats_kernel, dim3(static_cast<unsigned>((nseg + kMitThreads - 1) / kMitThreads)), dim3(kMitThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(mit_scan_kernel, dim3(1), dim3(kMitThreads), 0, ctx->stream, a);
    if (nseg > 0) {
        const int64_t blocks = std::min<int64_t>((nk + kMitThreads - 1) / kMitThreads, 1 << 16);
        hipLaunchKernelGGL(mit_apply_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kMitThreads), 0, ctx->stream, a);
        if (a.kind != GNSSHIP_MIT_PULSE_BLANKING) {
            if (m->chain_form == GNSSHIP_MIT_CHAIN_SPECULATIVE) {
                hipLaunchKernelGGL(mit_chain_spec_kernel, dim3(static_cast<unsigned>((a.nchunks + 63) / 64)), dim3(64), 0, ctx->stream, a);
                hipLaunchKernelGGL(mit_chain_fix_kernel, dim3(1), dim3(1), 0, ctx->stream, a);
            } else {
                hipLaunchKernelGGL(mit_chain_serial_kernel, dim3(static_cast<unsigned>((nseg + 63) / 64)), dim3(64), 0, ctx->stream, a);
            }
        }
    }
    if (int rc = launched(ctx, "gnsship_mit_run(launch)")) return rc;
    m->carry_cur ^= 1;
    m->cur ^= 1;
    m->n_pending = avail - nk;
    m->samples_in += static_cast<uint64_t>(n_in);
    m->samples_out += static_cast<uint64_t>(nk);
    if (dev_out) *dev_out = a.out;
    if (n_out) *n_out = nk;
    if (host_out && nk == 0) {  // a host run returns finished even when it emits nothing: copy_out would not wait
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, "gnsship_mit_run(download)");
    }
    return copy_out(ctx, {{host_out, a.out, sizeof(float2) * static_cast<size_t>(nk)}}, "gnsship_mit_run(download)");
}
