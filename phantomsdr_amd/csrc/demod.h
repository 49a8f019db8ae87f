// demod.h — batched per-client downconversion: frequency-domain slice -> small inverse
// DFT -> USB/LSB/AM/FM, with the 50 % overlap-add carried across frames.
//
// Replaces AudioClient::send_audio (src/signal.cpp:102-275) for all clients and all
// frames of a batch at once:
//   k_demod_idft  one work-group per (client, frame): average_power (:117-119), the
//                 mode-specific bin copy (:125-153, :175-198), the n-point backward
//                 transform (fftwf c2r / c2c, :138,154,214), LSB reversal (:155) and the
//                 odd-frame sign flip (:160-168, :223-234).
//   k_demod_ola   overlap-add with the previous frame's second half (:171-172,
//                 :235-237), AM envelope (dsp_am_demod, src/utils/dsp.cpp:116-126),
//                 FM polar discriminator (src/utils/dsp.cpp:27-35), NaN guard (:266-271)
//                 and the state carried to the next batch (:200-203, :273-275).
// The AM "carrier" transform (:205-222,230-241) feeds only the liquid-dsp PLL branch
// (:242-252), which is not part of the parity target: USB / LSB / AM / FM / IQ clients do not
// compute it.  PSDR_SAM clients do (k_demod_chain_sam / k_demod_ola_sam at the end of this
// file): the carrier baseband is their phase reference, feed-forward, in place of the PLL.
//
// n = audio_fft_size is any multiple of 4 (248, 360, 720, 10068 ...): the transform is
// a generic-radix Stockham, each radix-R butterfly a direct R-point DFT whose
// inter-stage twiddle is folded into a single table lookup:
//   y[j + s*p] = sum_q x[i + q*n/R] * W_n^{ q*(k + s*p)*n/(p*R) },  k = i mod p,
//   j = (i-k)*R + k,  W_n = exp(+2*pi*i/n)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "butterfly.h"
#include "quantize.h"
#include "types.h"

namespace psdr {



struct DemodArgs {
    const cf *spec;  // [nframes][spec_stride]; IQ: client order, real: k order, through `lay`
    size_t spec_stride;
    SpecLayout lay;  // where bin c of a frame sits (quantize.h); natural order unless the fused real path
    int is_real;
    int n;  // audio_fft_size
    int nframes;
    int max_batch;
    unsigned long long first_frame_num;
    const ClientParams *clients;  // compact list of active clients
    const cf *Wn;                 // exp(+2 pi i j / n), j < n
    int nstages;
    int radix[PSDR_MAX_STAGES];
    const int4 *stage_tab;  // [nstages][n]: {first input i, output index j+s*p, twiddle step e1, 0}
    cf *ypost;  // [slots][max_batch][n]: transform output after reversal/flip
    float *pwr;  // [slots][max_batch]
    // workspace for transforms too large for LDS: [gridDim.x*gridDim.y][2][n]
    cf *gscratch;
    int lds_mode;  // 0: bufA, bufB, Wn in LDS; 1: bufA, bufB in LDS; 2: all global
    // ola
    float *audio;  // [slots][max_batch][n/2]
    int *nan_flags;  // [slots][max_batch]
    float *real_prev;  // [2][slots][n/2]
    cf *bb_tail;       // [2][slots][n/2]
    cf *bb_last;       // [2][slots]
    int slots;
    // The NaN guard of USB / LSB (src/signal.cpp:266-275) is a recurrence over a client's frames: frame f is dropped iff
    // y_f[0..n/2) + prev has a NaN, and prev moves on only if it was not.  The batched kernels evaluate it per chain of frames
    // with "the frame before was dropped iff its transform carries NaN" - exact as long as every value is finite or a
    // transform is NaN throughout (a NaN input sample).  A client whose batch shows ANY non-finite value (an Inf sample, a
    // tail that went bad in an earlier batch) is marked here and walked again, strictly in frame order, by one wave
    // (`replay`: k_demod_chain_fixed with the whole batch as one chain / k_demod_ola_seq) - the reference's rule on the
    // values at hand, whatever they are.  Integer input formats never get there.
    unsigned *ssb_mark;   // [slots]: == mark_epoch: the slot's batch needs the sequential walk
    unsigned mark_epoch;  // of this batch (never 0)
    int replay;           // 1: the sequential walk itself (marked slots only)
    // Notches (include/psdr.h: psdr_client_set_notch / _set_auto_notch): half-open intervals [first, end) of spectrum bins, in
    // the coordinates of ClientParams::l / r, that a client's kernels take as +0.0 + 0.0i instead of loading them
    const int4 *notch_man;   // [slots] (first0, end0, first1, end1): the batch's snapshot of the manual notches, uploaded with the
                             // client list; null: no client of the batch has one
    const int4 *notch_auto;  // [slots] (first2, end2, first3, end3): the device-resident table k_notch_detect writes behind the
                             // batch's last demodulation kernel; null: no client of the context has ever switched auto-notch on
};
__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) <= 3.402823466e38f); }  // NaN or +-Inf

__device__ __forceinline__ bool flip_frame(unsigned long long frame_num, int m_idx, int is_real) {
    // src/signal.cpp:160-162 with C++ remainder semantics for negative m_idx
    return (frame_num % 2 == 1) && ((m_idx % 2 == 0 && !is_real) || (m_idx % 2 == 1 && is_real));
}
// s_f: the sign frame f of the batch is multiplied with
__device__ __forceinline__ float frame_sign(const DemodArgs &a, const ClientParams &cp, int f) {
    return flip_frame(a.first_frame_num + (unsigned long long)f, cp.m_floor, a.is_real) ? -1.f : 1.f;
}

// ---- steps the kernels below share: ONE definition each -----------------------------------------------------------------
// (The complex overlap-add step of the three chain kernels - y = s_f buf[j], b = y + tail, tail = s_f buf[h + j], the state on
// the batch's last frame - stays written out in each: as one function k_demod_chain_fixed<360> took 83 VGPRs, <720> 44 bytes
// of scratch and k_demod_chain_sam<360> 89 VGPRs, over their budgets beside a pass.  The kernels behind the IDFT share theirs:
// ola_step.)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// the twiddle table into the front of the work-group's LDS, behind the only work-group barrier of the wave-per-item kernels
__device__ __forceinline__ cf *stage_twiddles(const DemodArgs &a, unsigned char *smem, int n) {
    cf *Wn = reinterpret_cast<cf *>(smem);
    for (int i = threadIdx.x; i < n; i += blockDim.x) Wn[i] = a.Wn[i];
    __syncthreads();
    return Wn;
}
// wave -> item: wave wv of work-group b takes item b W + wv of nact * ceil(F / K), the chain [f0, f1) of K consecutive frames
// (the last one of a client may be shorter) of client ci; false: the grid's surplus.  Wave-uniform, in scalar registers.
__device__ __forceinline__ bool wave_chain(int nact, int F, int K, int &ci, int &f0, int &f1) {
    const int wv = threadIdx.x >> 6, W = blockDim.x >> 6, nch = (F + K - 1) / K;
    const int item = __builtin_amdgcn_readfirstlane((int)blockIdx.x * W + wv);
    if (item >= nact * nch) return false;
    ci = item / nch, f0 = (item - ci * nch) * K;
    f1 = f0 + K < F ? f0 + K : F;
    return true;
}
// everything about a wave's client is wave-uniform: keep it in scalar registers (the mode branches become scalar
// branches, the range tests compare against scalars)
__device__ __forceinline__ ClientParams wave_uniform(ClientParams cp) {
    cp.l = __builtin_amdgcn_readfirstlane(cp.l);
    cp.r = __builtin_amdgcn_readfirstlane(cp.r);
    cp.m_floor = __builtin_amdgcn_readfirstlane(cp.m_floor);
    cp.mode = __builtin_amdgcn_readfirstlane(cp.mode);
    cp.slot = __builtin_amdgcn_readfirstlane(cp.slot);
    cp.state_cur = __builtin_amdgcn_readfirstlane(cp.state_cur);
    return cp;
}
// A client's notches: up to four half-open intervals of spectrum bins, wave-uniform, in scalar registers (an empty entry is
// 0, 0).  `any`: one of them is set - a client without notches passes every test with one scalar compare.
struct Notches {
    int f0, e0, f1, e1, f2, e2, f3, e3;
    int any;
};
__device__ __forceinline__ Notches notch_load(const DemodArgs &a, int slot) {
    int4 m = make_int4(0, 0, 0, 0), t = make_int4(0, 0, 0, 0);
    if (a.notch_man) m = a.notch_man[slot];
    if (a.notch_auto) t = a.notch_auto[slot];
    Notches nz;
    nz.f0 = __builtin_amdgcn_readfirstlane(m.x), nz.e0 = __builtin_amdgcn_readfirstlane(m.y);
    nz.f1 = __builtin_amdgcn_readfirstlane(m.z), nz.e1 = __builtin_amdgcn_readfirstlane(m.w);
    nz.f2 = __builtin_amdgcn_readfirstlane(t.x), nz.e2 = __builtin_amdgcn_readfirstlane(t.y);
    nz.f3 = __builtin_amdgcn_readfirstlane(t.z), nz.e3 = __builtin_amdgcn_readfirstlane(t.w);
    nz.any = (nz.e0 > nz.f0) | (nz.e1 > nz.f1) | (nz.e2 > nz.f2) | (nz.e3 > nz.f3);
    return nz;
}
// "is slice bin t of this client notched": THE definition - every place a kernel reads a client's spectrum bins asks it
// and takes +0.0 + 0.0i for a notched bin instead of loading it.  (The defining rule of include/psdr.h follows: whatever is
// computed from the bins is computed from a spectrum whose notched bins are zero.)
__device__ __forceinline__ bool notched(const Notches &nz, const ClientParams &cp, int t) {
    const int b = cp.l + t;
    return nz.any && ((b >= nz.f0 && b < nz.e0) || (b >= nz.f1 && b < nz.e1) || (b >= nz.f2 && b < nz.e2) || (b >= nz.f3 && b < nz.e3));
}
// ... loaded again for every frame of a chain, behind an opaque copy of the slot (two scalar loads that hit the constant
// cache): held across the frame loop the nine scalars pushed k_demod_chain_sam<720> and k_demod_chain_sbsam<720> into 12
// bytes of scratch (scalar registers spilled into vector lanes) - DESIGN.md 3.11
__device__ __forceinline__ Notches notch_load_frame(const DemodArgs &a, int slot) {
    asm volatile("" : "+s"(slot));
    return notch_load(a, slot);
}
// a client's double-buffered state (src/signal.h:86-101): this batch reads half state_cur and writes the other one
struct SlotState {
    size_t row_old, row_new;  // [half][slot]: the element of bb_last, the row of real_prev / bb_tail / SamArgs::car_tail
    const float *rp_old;
    float *rp_new;
    const cf *bt_old;
    cf *bt_new;
};
__device__ __forceinline__ SlotState slot_state(const DemodArgs &a, const ClientParams &cp, int h) {
    const size_t srow = (size_t)cp.slot;
    const int cur = cp.state_cur, nxt = cur ^ 1;
    SlotState st;
    st.row_old = (size_t)cur * a.slots + srow;
    st.row_new = (size_t)nxt * a.slots + srow;
    st.rp_old = a.real_prev + ((size_t)cur * a.slots + srow) * h;
    st.rp_new = a.real_prev + ((size_t)nxt * a.slots + srow) * h;
    st.bt_old = a.bb_tail + ((size_t)cur * a.slots + srow) * h;
    st.bt_new = a.bb_tail + ((size_t)nxt * a.slots + srow) * h;
    return st;
}
// An opaque copy of the lane number for one iteration of a chain kernel's frame loop: with the loop-invariant lane the
// compiler keeps every address of every stage in registers across the loop - 100 VGPRs more than the transform itself
// needs, or 300-700 bytes of scratch
__device__ __forceinline__ int opaque_lane(int lane) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    return ln;
}

// one Stockham stage; RC > 0: radix known at compile time (all operand loads of a butterfly
// are issued before the MAC chain), RC == 0: run-time radix (large prime factors)
template <int RC>
__device__ __forceinline__ void idft_stage(const cf *src, cf *dst, const cf *Wn, const int4 *tab, int n,
                                           int R, int tid, int NT) {
    const int tlen = n / R;
    for (int o = tid; o < n; o += NT) {
        const int4 tb = tab[o];
        const int e1 = tb.z;
        const cf *xp = src + tb.x;
        float ar = 0.f, ai = 0.f;
        if constexpr (RC > 0) {
            // operands in groups of 4: enough loads in flight, few registers (the kernel shares
            // the SIMDs' register file with the FFT passes: <= 48 VGPRs doubles its occupancy)
            int e = 0;
#pragma unroll
            for (int q0 = 0; q0 < RC; q0 += 4) {
                constexpr int G = 4;
                cf x[G], w[G];
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (q0 + g < RC) {
                        x[g] = xp[(q0 + g) * tlen];
                        w[g] = Wn[e];
                        e += e1;
                        if (e >= n) e -= n;
                    }
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (q0 + g < RC) {
                        ar = fmaf(x[g].x, w[g].x, fmaf(-x[g].y, w[g].y, ar));
                        ai = fmaf(x[g].x, w[g].y, fmaf(x[g].y, w[g].x, ai));
                    }
            }
        } else {
            int e = 0;
#pragma unroll 4
            for (int q = 0; q < R; q++) {
                const cf x = xp[q * tlen];
                const cf w = Wn[e];
                ar = fmaf(x.x, w.x, fmaf(-x.y, w.y, ar));
                ai = fmaf(x.x, w.y, fmaf(x.y, w.x, ai));
                e += e1;
                if (e >= n) e -= n;
            }
        }
        dst[tb.y] = make_float2(ar, ai);
    }
}

// The transform of ONE (client, frame) item into its row of ypost by the NT threads that share bufA / bufB: slice power,
// the mode-specific bin copy, the c2r extension, the stages, reversal (LSB) and sign.  `sy` is how these threads pass a
// stage boundary together and sum the power: ItemGroup (a work-group: barriers) or ItemWave (one wave: its LDS
// operations execute in order).
struct ItemGroup {
    float *red;  // [NT / 64] in LDS
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // the item's power from the waves' sums (in thread 0), behind a boundary
    __device__ __forceinline__ float total(float pw, int tid, int NT) const {
        if ((tid & 63) == 0) red[tid >> 6] = pw;
        __syncthreads();
        float tot = 0.f;
        if (tid == 0)
            for (int w = 0; w < NT / 64; w++) tot += red[w];
        return tot;
    }
};
struct ItemWave {
    __device__ __forceinline__ void sync() const { wave_lds_sync(); }
    __device__ __forceinline__ float total(float pw, int, int) const {
        wave_lds_sync();
        return pw;
    }
};
template <class Sync>
__device__ __forceinline__ void idft_item(const DemodArgs &a, const ClientParams &cp, int f, cf *bufA, cf *bufB, const cf *Wn,
                                          int tid, int NT, Sync sy) {
    const int n = a.n;
    const int len = cp.r - cp.l;
    const int m = cp.m_floor - cp.l;  // audio_m
    const cf *S = a.spec + (size_t)f * a.spec_stride;  // slice bin t at lay.pos(cp.l + t)
    const Notches nz = notch_load(a, cp.slot);

    for (int i = tid; i < n; i += NT) bufA[i] = make_float2(0.f, 0.f);
    sy.sync();

    float pw = 0.f;
    for (int t = tid; t < len; t += NT) {
        const cf v = notched(nz, cp, t) ? make_float2(0.f, 0.f) : S[a.lay.pos(cp.l + t)];
        pw += fmaf(v.x, v.x, v.y * v.y);
        if (cp.mode == 0) {  // USB :125-137
            if (t >= m && t < m + n) bufA[t - m] = v;
        } else if (cp.mode == 1) {  // LSB :139-153
            if (t >= m - n + 1 && t < m + 1) bufA[m - t] = v;
        } else {  // AM/FM :175-198
            if (t >= m && t < m + n / 2) bufA[t - m] = v;
            if (t >= m - n / 2 + 1 && t < m) bufA[n - m + t] = v;
        }
    }
    const float tot = sy.total(wave_sum(pw), tid, NT);
    if (tid == 0) a.pwr[(size_t)cp.slot * a.max_batch + f] = tot;

    if (cp.mode < 2) {
        // c2r semantics: bins 0..n/2 only, Im of bin 0 and bin n/2 ignored; extend to the
        // Hermitian-symmetric full spectrum so the complex transform returns the real signal
        for (int k = tid + 1; k < n / 2; k += NT) {
            const cf v = bufA[k];
            bufA[n - k] = make_float2(v.x, -v.y);
        }
        if (tid == 0) {
            bufA[0].y = 0.f;
            bufA[n / 2].y = 0.f;
        }
        sy.sync();
    }

    // generic-radix Stockham, backward; the index arithmetic of every (stage, output) pair is
    // precomputed on the host (stage_tab), the butterfly is R complex MACs
    cf *src = bufA, *dst = bufB;
    for (int st = 0; st < a.nstages; st++) {
        const int R = a.radix[st];
        const int4 *tab = a.stage_tab + (size_t)st * n;
        switch (R) {
#define PSDR_RCASE(r) case r: idft_stage<r>(src, dst, Wn, tab, n, r, tid, NT); break;
            PSDR_RCASE(2) PSDR_RCASE(3) PSDR_RCASE(4) PSDR_RCASE(5) PSDR_RCASE(6) PSDR_RCASE(7)
            PSDR_RCASE(8) PSDR_RCASE(9) PSDR_RCASE(10) PSDR_RCASE(12) PSDR_RCASE(14)
            PSDR_RCASE(15) PSDR_RCASE(16)
#undef PSDR_RCASE
            default: idft_stage<0>(src, dst, Wn, tab, n, R, tid, NT); break;
        }
        cf *tmp = src;
        src = dst;
        dst = tmp;
        sy.sync();
    }

    const float sg = frame_sign(a, cp, f);
    cf *yp = a.ypost + ((size_t)cp.slot * a.max_batch + f) * n;
    for (int jx = tid; jx < n; jx += NT) {
        cf v;
        if (cp.mode == 0)
            v = make_float2(src[jx].x * sg, 0.f);
        else if (cp.mode == 1)
            v = make_float2(src[n - 1 - jx].x * sg, 0.f);  // std::reverse :155
        else
            v = make_float2(src[jx].x * sg, src[jx].y * sg);
        yp[jx] = v;
    }
}

// one work-group per (client, frame); blockDim.x = 128 (n <= 512) or 256
__global__ __launch_bounds__(256) void k_demod_idft(DemodArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = a.n, tid = threadIdx.x, NT = blockDim.x;
    cf *bufA, *bufB;
    const cf *Wn;
    if (a.lds_mode == 0) {
        bufA = reinterpret_cast<cf *>(smem);
        bufB = bufA + n;
        cf *w = bufB + n;
        for (int i = tid; i < n; i += NT) w[i] = a.Wn[i];  // (idft_item's first boundary covers it)
        Wn = w;
    } else if (a.lds_mode == 1) {
        bufA = reinterpret_cast<cf *>(smem);
        bufB = bufA + n;
        Wn = a.Wn;
    } else {
        bufA = a.gscratch + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 2) * n;
        bufB = bufA + n;
        Wn = a.Wn;
    }
    __shared__ float red[4];
    idft_item(a, a.clients[blockIdx.x], blockIdx.y, bufA, bufB, Wn, tid, NT, ItemGroup{red});
}

// The same transform with one WAVE per (client, frame) and no work-group barrier: the 64
// lanes of a wave execute their LDS operations in order, so a stage boundary is just
// "s_waitcnt lgkmcnt(0)".  With hundreds of clients the one-work-group-per-item kernel above
// is bound by its ~10 barriers per item while it shares the CUs with the persistent FFT
// passes; here a 128-thread work-group carries two independent items in < 16 KiB of LDS (the
// space an FFT pass leaves free on a CU).  n <= 512 (audio_fft_size 248, 360, ...).
//   grid = ceil(nact * nframes / WAVES); dynamic LDS = (2 * WAVES + 1) * n * 8 bytes
#define PSDR_IDFT_WAVES 2
__global__ __launch_bounds__(64 * PSDR_IDFT_WAVES) void k_demod_idft_wave(DemodArgs a, int nact) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = a.n, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cf *Wn = stage_twiddles(a, smem, n);
    const int item = blockIdx.x * PSDR_IDFT_WAVES + wv;
    if (item >= nact * a.nframes) return;
    // consecutive items = consecutive frames of one client: the slice addresses of a
    // work-group's waves are F*8N bytes apart, their table look-ups identical
    const int ci = item / a.nframes, f = item - ci * a.nframes;
    cf *bufA = Wn + n + (size_t)wv * 2 * n, *bufB = bufA + n;
    idft_item(a, a.clients[ci], f, bufA, bufB, Wn, lane, 64, ItemWave{});
}

// ---- compile-time plans for the audio sizes the BASELINE configurations use (n = 360, 720)
// The generic kernels above spend most of their ~2000 wave instructions per 360-point item on
// index arithmetic, table look-ups and predication, and with hundreds of clients the
// demodulation is VALU-issue bound (65 536 items: 227 us on an idle chip, 1.5-2x that beside
// the FFT passes).  Here n and the radices are template parameters: a lane owns whole radix-R
// butterflies (R inputs read once, outputs from registers with the R-th roots, conjugate pairs
// (s, R-s) sharing their sums), every LDS access is base + immediate, the twiddle exponent
// q*(i%p)*n/(p*R) never wraps, and each stage runs IN PLACE (all reads of a stage precede its
// first write; LDS operations of one wave execute in order) so four items share 15 KiB.
// ---- in-register INVERSE (sign +) butterflies of the compile-time plans: x[s] <- sum_q x[q] exp(+2 pi i q s / R) ----------
// Round 5's stage computed every butterfly as a direct R-point DFT (conjugate pairs sharing their sums: ~R^2 scalar FMAs -
// 124 / 160 / 48 instructions for R = 8 / 9 / 5), and with hundreds of clients the demodulation is VALU-bound beside the
// passes (1024 clients: a third of the step).  Here R = 8 = 2.2.2, 9 = 3.3, 5 (the symmetric form) and 10 = 2.5 with literal
// roots on packed (re, im) pairs: 30 / 44 / 18 packed instructions.  butterfly.h's add_mi(a, d) = a - i d, sub_mi(a, d) = a + i d.
__device__ __forceinline__ cf id_scale(cf a, float k) { return make_float2(a.x * k, a.y * k); }
__device__ __forceinline__ cf id_fma(cf a, float k, cf c) { return make_float2(fmaf(a.x, k, c.x), fmaf(a.y, k, c.y)); }  // a k + c
__device__ __forceinline__ void idft3(cf &x0, cf &x1, cf &x2) {
    constexpr float S3 = 0.86602540378443864676f;  // sin(2 pi / 3)
    const cf t = cadd(x1, x2), d = csub(x1, x2);
    const cf u = id_fma(t, -0.5f, x0), e = id_scale(d, S3);
    x0 = cadd(x0, t);
    x1 = sub_mi(u, e);  // u + i e
    x2 = add_mi(u, e);  // u - i e
}
__device__ __forceinline__ void idft4(cf &x0, cf &x1, cf &x2, cf &x3) {
    const cf s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = csub(x1, x3);
    x0 = cadd(s02, s13);
    x2 = csub(s02, s13);
    x1 = sub_mi(d02, d13);  // d02 + i d13
    x3 = add_mi(d02, d13);
}
__device__ __forceinline__ void idft5(cf &x0, cf &x1, cf &x2, cf &x3, cf &x4) {
    constexpr float C1 = 0.30901699437494742410f, C2 = -0.80901699437494742410f;   // cos(2 pi / 5), cos(4 pi / 5)
    constexpr float S1 = 0.95105651629515357212f, S2 = 0.58778525229247312917f;    // sin(2 pi / 5), sin(4 pi / 5)
    const cf t1 = cadd(x1, x4), t2 = cadd(x2, x3), d1 = csub(x1, x4), d2 = csub(x2, x3);
    const cf a1 = id_fma(t2, C2, id_fma(t1, C1, x0)), a2 = id_fma(t2, C1, id_fma(t1, C2, x0));
    const cf b1 = id_fma(d2, S2, id_scale(d1, S1)), b2 = id_fma(d2, -S1, id_scale(d1, S2));
    x0 = cadd(x0, cadd(t1, t2));
    x1 = sub_mi(a1, b1);
    x4 = add_mi(a1, b1);
    x2 = sub_mi(a2, b2);
    x3 = add_mi(a2, b2);
}
template <int R>
__device__ __forceinline__ void idft_bfly(cf (&x)[R]) {
    if constexpr (R == 5) {
        idft5(x[0], x[1], x[2], x[3], x[4]);
    } else if constexpr (R == 8) {
        // q = 2 q1 + q2, s = s1 + 4 s2: four-point transforms of the even and the odd inputs, odd branch times W8^{s1}
        idft4(x[0], x[2], x[4], x[6]);
        idft4(x[1], x[3], x[5], x[7]);
        const cf e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6], o0 = x[1], o2 = x[5];
        const cf o1 = id_scale(sub_mi(x[3], x[3]), PSDR_SQRT1_2);  // (1 + i) / sqrt 2 * o1
        const cf t3 = id_scale(sub_mi(x[7], x[7]), PSDR_SQRT1_2);  // W8^3 o3 = i * this
        x[0] = cadd(e0, o0);
        x[4] = csub(e0, o0);
        x[1] = cadd(e1, o1);
        x[5] = csub(e1, o1);
        x[2] = sub_mi(e2, o2);  // + i o2
        x[6] = add_mi(e2, o2);
        x[3] = sub_mi(e3, t3);
        x[7] = add_mi(e3, t3);
    } else if constexpr (R == 9) {
        // q = 3 q1 + q2, s = s1 + 3 s2: three-point transforms over q1, y[s1][q2] *= W9^{q2 s1}, three-point transforms over q2
        idft3(x[0], x[3], x[6]);
        idft3(x[1], x[4], x[7]);
        idft3(x[2], x[5], x[8]);
        const cf w1 = make_float2(0.76604444311897803520f, 0.64278760968653932632f);   // exp(+2 pi i 1/9)
        const cf w2 = make_float2(0.17364817766693034885f, 0.98480775301220805937f);   // exp(+2 pi i 2/9)
        const cf w4 = make_float2(-0.93969262078590838405f, 0.34202014332566873304f);  // exp(+2 pi i 4/9)
        // after the first step x[3 s1 + q2] holds y[s1][q2]
        cmul_pair(x[4], x[4], w1, x[5], x[5], w2);
        cmul_pair(x[7], x[7], w2, x[8], x[8], w4);
        idft3(x[0], x[1], x[2]);  // s1 = 0: X[0], X[3], X[6]
        idft3(x[3], x[4], x[5]);  // s1 = 1: X[1], X[4], X[7]
        idft3(x[6], x[7], x[8]);  // s1 = 2: X[2], X[5], X[8]
        // x[3 s1 + s2] = X[s1 + 3 s2]: transpose to natural order
        cf t;
        t = x[1], x[1] = x[3], x[3] = t;
        t = x[2], x[2] = x[6], x[6] = t;
        t = x[5], x[5] = x[7], x[7] = t;
    } else {
        static_assert(R == 10, "butterflies with literal roots: 5, 8, 9, 10");
        // q = 2 q1 + q2, s = s1 + 5 s2
        idft5(x[0], x[2], x[4], x[6], x[8]);
        idft5(x[1], x[3], x[5], x[7], x[9]);
        const cf w1 = make_float2(0.80901699437494742410f, 0.58778525229247312917f);   // exp(+2 pi i 1/10)
        const cf w2 = make_float2(0.30901699437494742410f, 0.95105651629515357212f);
        const cf w3 = make_float2(-0.30901699437494742410f, 0.95105651629515357212f);
        const cf w4 = make_float2(-0.80901699437494742410f, 0.58778525229247312917f);
        cf o1, o2, o3, o4;
        cmul_pair(o1, x[3], w1, o2, x[5], w2);
        cmul_pair(o3, x[7], w3, o4, x[9], w4);
        const cf e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6], e4 = x[8], o0 = x[1];
        x[0] = cadd(e0, o0), x[5] = csub(e0, o0);
        x[1] = cadd(e1, o1), x[6] = csub(e1, o1);
        x[2] = cadd(e2, o2), x[7] = csub(e2, o2);
        x[3] = cadd(e3, o3), x[8] = csub(e3, o3);
        x[4] = cadd(e4, o4), x[9] = csub(e4, o4);
    }
}

template <int N, int R, int PP>
__device__ __forceinline__ void idft_stage_fixed(cf *buf, const cf *Wn, int lane) {
    constexpr int TLEN = N / R, ROUNDS = (TLEN + 63) / 64, STEP = N / (PP * R);
    constexpr bool RAGGED = (TLEN % 64) != 0;
    cf x[ROUNDS][R];
    int jo[ROUNDS];
#pragma unroll
    for (int rr = 0; rr < ROUNDS; rr++) {
        const int i = lane + 64 * rr;
        if (!RAGGED || rr + 1 < ROUNDS || i < TLEN) {
            const int k = PP == 1 ? 0 : i % PP;
            jo[rr] = (i - k) * R + k;
            x[rr][0] = buf[i];
#pragma unroll
            for (int q = 1; q < R; q++) {
                const cf v = buf[i + q * TLEN];
                if (PP > 1)
                    x[rr][q] = cmul(v, Wn[q * k * STEP]);
                else
                    x[rr][q] = v;
            }
        }
    }
    // Compiler barrier, no hardware wait: the LDS executes a wave's operations in order, but the
    // compiler reasons per lane - with compile-time indices it can prove that a lane's own
    // loads and stores never overlap and sink the later rounds' loads below the first stores,
    // which other LANES' stores then clobber (seen as 0.4 % errors in 40 outputs of n = 360).
    asm volatile("" ::: "memory");
#pragma unroll
    for (int rr = 0; rr < ROUNDS; rr++) {
        const int i = lane + 64 * rr;
        if (!RAGGED || rr + 1 < ROUNDS || i < TLEN) {
            cf *o = buf + jo[rr];
            idft_bfly<R>(x[rr]);
#pragma unroll
            for (int s = 0; s < R; s++) o[s * PP] = x[rr][s];
        }
    }
}

// the transform of ONE (client, frame) item by one wave: slice load, mode-specific bin copy, c2r symmetry, the
// stages.  Leaves the n outputs in buf (before reversal / sign flip) and returns the slice power (all lanes).
// the slice of one (client, frame) item, bin t = lane + 64 u in sv[u] (at most n bins, src/signal.cpp:309-311)
template <int N>
__device__ __forceinline__ void idft_load_slice(const DemodArgs &a, const ClientParams &cp, const Notches &nz, int f, int lane, cf (&sv)[(N + 63) / 64]) {
    const int len = cp.r - cp.l;
    const cf *S = a.spec + (size_t)f * a.spec_stride;  // slice bin t at lay.pos(cp.l + t)
#pragma unroll
    for (int u = 0; u < (N + 63) / 64; u++) {
        const int t = lane + 64 * u;
        sv[u] = t < len && !notched(nz, cp, t) ? S[a.lay.pos(cp.l + t)] : make_float2(0.f, 0.f);
    }
}
// the same in two steps for a wave that walks SEVERAL frames of one client: where bin t of the slice sits inside a frame
// (SpecLayout::pos: ~25 instructions per bin in the tile-major layouts) does not depend on the frame - computed once per
// chain, a frame's load is base + offset (k_demod_chain_fixed: a fifth of its instructions per frame were these).  The
// first HO rounds of 64 bins only (registers: the kernel lives in the ~80 a pass leaves per SIMD lane): slices of up to
// 64 HO bins - every SSB / AM / FM window of the usual widths - never compute a position inside the frame loop
template <int N, int HO>
__device__ __forceinline__ void idft_slice_offsets(const DemodArgs &a, const ClientParams &cp, int lane, unsigned (&so)[HO]) {
    const int len = cp.r - cp.l;
#pragma unroll
    for (int u = 0; u < HO; u++) {
        const int t = lane + 64 * u;
        so[u] = t < len ? (unsigned)a.lay.pos(cp.l + t) : 0u;  // (element index inside a frame / band region: < 2^32)
    }
}
// (NZ = false: the notch test left out - k_demod_chain_iq, which has neither a vector nor a scalar register to spare; its
// twin k_demod_chain_iq_nz serves the lists that contain a notched client)
template <int N, int HO, bool NZ = true>
__device__ __forceinline__ void idft_load_slice_at(const DemodArgs &a, const ClientParams &cp, const Notches &nz, int f, const unsigned (&so)[HO], int lane, cf (&sv)[(N + 63) / 64]) {
    const int len = cp.r - cp.l;
    const cf *S = a.spec + (size_t)f * a.spec_stride;
#pragma unroll
    for (int u = 0; u < (N + 63) / 64; u++) {
        const int t = lane + 64 * u;
        const bool in = t < len && !(NZ && notched(nz, cp, t));
        if (u < HO)
            sv[u] = in ? S[so[u]] : make_float2(0.f, 0.f);
        else
            sv[u] = in ? S[a.lay.pos(cp.l + t)] : make_float2(0.f, 0.f);
    }
}
template <int N, int R0, int R1, int R2>
__device__ __forceinline__ float idft_slice_fixed(const ClientParams &cp, const cf (&sv)[(N + 63) / 64], cf *buf, const cf *Wn, int lane);
template <int N, int R0, int R1, int R2>
__device__ __forceinline__ float idft_item_fixed(const DemodArgs &a, const ClientParams &cp, int f, cf *buf, const cf *Wn, int lane) {
    cf sv[(N + 63) / 64];  // loads first, LDS after
    idft_load_slice<N>(a, cp, notch_load(a, cp.slot), f, lane, sv);
    return idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
}
template <int N, int R0, int R1, int R2>
__device__ __forceinline__ float idft_slice_fixed(const ClientParams &cp, const cf (&sv)[(N + 63) / 64], cf *buf, const cf *Wn, int lane) {
    const int len = cp.r - cp.l;
    const int m = cp.m_floor - cp.l;  // audio_m
    constexpr int NR = (N + 63) / 64;
#pragma unroll
    for (int u = 0; u < NR; u++) {
        const int i = lane + 64 * u;
        if (i < N) buf[i] = make_float2(0.f, 0.f);
    }
    asm volatile("" ::: "memory");  // zero-fill before any lane's scatter (compiler order, see above)
    float pw = 0.f;
#pragma unroll
    for (int u = 0; u < NR; u++) {
        const int t = lane + 64 * u;
        if (t < len) {
            const cf v = sv[u];
            pw += fmaf(v.x, v.x, v.y * v.y);
            // USB / LSB are c2r transforms (fftwf_plan_dft_c2r_1d, src/signal.cpp:138, 154): only bins 0..N/2 of the input
            // array are read, Im of bins 0 and N/2 is ignored, the rest is the Hermitian mirror.  The scatter writes a bin
            // AND its mirror (round 5: a second pass over the buffer behind an LDS round trip)
            if (cp.mode < 2) {
                const int idx = cp.mode == 0 ? t - m : m - t;  // USB :125-137 / LSB :139-153
                if (idx == 0 || idx == N / 2) {
                    buf[idx] = make_float2(v.x, 0.f);
                } else if (idx > 0 && idx < N / 2) {
                    buf[idx] = v;
                    buf[N - idx] = make_float2(v.x, -v.y);
                }
            } else {  // AM/FM :175-198
                if (t >= m && t < m + N / 2) buf[t - m] = v;
                if (t >= m - N / 2 + 1 && t < m) buf[N - m + t] = v;
            }
        }
    }
    pw = wave_sum(pw);
    wave_lds_sync();
    idft_stage_fixed<N, R0, 1>(buf, Wn, lane);
    wave_lds_sync();
    idft_stage_fixed<N, R1, R0>(buf, Wn, lane);
    wave_lds_sync();
    if constexpr (R2 > 1) {
        idft_stage_fixed<N, R2, R0 * R1>(buf, Wn, lane);
        wave_lds_sync();
    }
    return pw;
}

//   grid = ceil(nact * nframes / W), W = blockDim.x / 64 items per work-group;
//   dynamic LDS = (1 + W) * N * 8 bytes
template <int N, int R0, int R1, int R2>
#ifndef PSDR_IDFT_WPE
#define PSDR_IDFT_WPE 5
#endif
__global__ __launch_bounds__(256, PSDR_IDFT_WPE) void k_demod_idft_fixed(DemodArgs a, int nact) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    int ci, f, f1;  // a chain of one frame
    if (!wave_chain(nact, a.nframes, 1, ci, f, f1)) return;
    const ClientParams cp = wave_uniform(a.clients[ci]);
    cf *buf = Wn + N + (size_t)wv * N;

    const float pw = idft_item_fixed<N, R0, R1, R2>(a, cp, f, buf, Wn, lane);
    if (lane == 0) a.pwr[(size_t)cp.slot * a.max_batch + f] = pw;
    constexpr int NR = (N + 63) / 64;
    const float sg = frame_sign(a, cp, f);
    cf *yp = a.ypost + ((size_t)cp.slot * a.max_batch + f) * N;
    // (mode is a scalar: one plain loop per mode.  The single unrolled loop with the three-way
    // per-lane select inside was miscompiled by this toolchain - the real part of the last,
    // partial round was read through a stale address register in the complex modes.)
    if (cp.mode == 0) {
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int jx = lane + 64 * u;
            if (jx < N) yp[jx] = make_float2(buf[jx].x * sg, 0.f);
        }
    } else if (cp.mode == 1) {
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int jx = lane + 64 * u;
            if (jx < N) yp[jx] = make_float2(buf[N - 1 - jx].x * sg, 0.f);  // std::reverse :155
        }
    } else {
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int jx = lane + 64 * u;
            if (jx < N) yp[jx] = make_float2(buf[jx].x * sg, buf[jx].y * sg);
        }
    }
}

// One complex overlap-add step behind the IDFT kernels (src/signal.cpp:235-237, 200-203), sample j < h of frame f of a
// client whose rows of ypost start at yp: b = y_f[j] + y_{f-1}[h + j] (the batch's first frame: the carried tail) -> use(b);
// on the batch's last frame the state the next batch starts from - the second half, B'_f[h-1] (`prev` of :200) - with
// USB / LSB's copied through.
template <class Use>
__device__ __forceinline__ void ola_step(const DemodArgs &a, const SlotState &st, const cf *yp, int f, int j, Use use) {
    const int n = a.n, h = n / 2;
    const cf *y = yp + (size_t)f * n;
    const cf pv = (f == 0) ? st.bt_old[j] : yp[(size_t)(f - 1) * n + h + j];
    const cf b = make_float2(y[j].x + pv.x, y[j].y + pv.y);  // dsp_add_complex :235
    use(b);
    if (f == a.nframes - 1) {
        st.bt_new[j] = y[h + j];  // :200-203 (second half kept for the next frame)
        st.rp_new[j] = st.rp_old[j];
        if (j == h - 1) a.bb_last[st.row_new] = b;  // `prev` of :200
    }
}

// one WAVE per (client, group of PSDR_OLA_FG consecutive frames): no shared memory, no barrier (NaN flag by
// wave vote).  A wave's life is three dependent round trips to memory (client parameters, then the two
// halves it adds, then the stores) whatever it does in between - with one frame per wave 65 536 waves of
// ~10 us each passed through the few wave slots the FFT passes leave free (256 clients x 256 frames:
// 700-800 us); a group of frames shares the parameter load and has all its loads in flight together.
// grid = ceil(nact * ceil(nframes / FG) / 4) work-groups of 256 threads
#ifndef PSDR_OLA_FG
#define PSDR_OLA_FG 8
#endif
__global__ __launch_bounds__(256) void k_demod_ola(DemodArgs a, int nact) {
    constexpr int FG = PSDR_OLA_FG;
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int F = a.nframes, ngrp = (F + FG - 1) / FG;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nact * ngrp) return;
    const int ci = item / ngrp;
    const ClientParams cp = a.clients[ci];
    const int f0 = (item - ci * ngrp) * FG;
    const size_t srow = (size_t)cp.slot;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;  // this client's frames
    const SlotState st = slot_state(a, cp, h);
#pragma unroll
    for (int g = 0; g < FG; g++) {
        const int f = f0 + g;
        if (f >= F) break;
        const cf *y = yp + (size_t)f * n;
        float *out = a.audio + (srow * a.max_batch + f) * h;
        int s_nan = 0;  // per lane; combined by a wave vote at the end
        const bool last = (f == F - 1);
        if (cp.mode < 2) {
            // the half to add is the second half of the latest EARLIER frame that survived the NaN guard: a dropped
            // frame throws at src/signal.cpp:266-271, before audio_real_prev is replaced (:273-275).  With finite values
            // nothing is ever dropped, and a NaN input sample makes a transform NaN throughout: "frame g was dropped" is
            // then read off the half that is loaded anyway.  Anything else non-finite: the slot is marked and
            // k_demod_ola_seq walks its batch in frame order afterwards (DemodArgs::ssb_mark).
            {
                int bad = 0;
                for (int j = tid; j < n; j += NT) bad |= not_finite(y[j].x) ? 1 : 0;
                if (f == 0)
                    for (int j = tid; j < h; j += NT) bad |= not_finite(st.rp_old[j]) ? 1 : 0;
                if (__any(bad) && tid == 0) a.ssb_mark[srow] = a.mark_epoch;
            }
            int g = f - 1;
            while (g >= 0) {
                int d = 0;
                for (int j = tid; j < h; j += NT) d |= isnan(yp[(size_t)g * n + h + j].x) ? 1 : 0;
                if (!__any(d)) break;
                g--;
            }
            for (int j = tid; j < h; j += NT) {
                const float prev = (g < 0) ? st.rp_old[j] : yp[(size_t)g * n + h + j].x;
                const float v = y[j].x + prev;  // dsp_add_float :171
                out[j] = v;
                if (isnan(v)) s_nan = 1;
            }
            if (last) {
                const int dropped = __any(s_nan);
                for (int j = tid; j < h; j += NT) {
                    // :273-275, unless this frame was dropped: then the tail it would have added stays
                    st.rp_new[j] = dropped ? ((g < 0) ? st.rp_old[j] : yp[(size_t)g * n + h + j].x) : y[h + j].x;
                    st.bt_new[j] = st.bt_old[j];
                }
                if (tid == 0) a.bb_last[st.row_new] = a.bb_last[st.row_old];
            }
        } else {
            for (int j = tid; j < h; j += NT)
                ola_step(a, st, yp, f, j, [&](cf b) {
                    float v;
                    if (cp.mode == 2) {
                        v = sqrtf(fmaf(b.x, b.x, b.y * b.y));  // dsp_am_demod
                    } else {
                        cf pr;
                        if (j > 0) {
                            const cf pv1 = (f == 0) ? st.bt_old[j - 1] : yp[(size_t)(f - 1) * n + h + j - 1];
                            pr = make_float2(y[j - 1].x + pv1.x, y[j - 1].y + pv1.y);
                        } else if (f == 0) {
                            pr = a.bb_last[st.row_old];
                        } else {
                            // B'_{f-1}[h-1] = y_{f-1}[h-1] + (tail of frame f-2, or the carried tail)
                            const cf y1 = yp[(size_t)(f - 1) * n + h - 1];
                            const cf t1 = (f == 1) ? st.bt_old[h - 1] : yp[(size_t)(f - 2) * n + n - 1];
                            pr = make_float2(y1.x + t1.x, y1.y + t1.y);
                        }
                        // arg(b * conj(pr)), src/utils/dsp.cpp:32
                        const float re = fmaf(b.x, pr.x, b.y * pr.y);
                        const float im = fmaf(b.x, -pr.y, b.y * pr.x);
                        v = atan2f(im, re);
                    }
                    out[j] = v;
                    if (isnan(v)) s_nan = 1;
                });
        }
        const int any_nan = __any(s_nan);
        if (tid == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
    }
}

// The NaN guard of USB / LSB as the recurrence it is (src/signal.cpp:266-275), for the slots k_demod_ola marked: one wave
// per client walks the batch in frame order - v = y_f[0..h) + prev; dropped iff v has a NaN; prev = y_f[h..n) unless dropped -
// and writes audio, flags and the carried tail again.  grid = ceil(nact / 4) work-groups of 256 threads.
__global__ __launch_bounds__(256) void k_demod_ola_seq(DemodArgs a, int nact) {
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ci >= nact) return;
    const ClientParams cp = a.clients[ci];
    const size_t srow = (size_t)cp.slot;
    if (cp.mode >= 2 || a.ssb_mark[srow] != a.mark_epoch) return;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;
    const SlotState st = slot_state(a, cp, h);
    int g = -1;  // the latest frame that survived (-1: the carried tail)
    for (int f = 0; f < a.nframes; f++) {
        const cf *y = yp + (size_t)f * n;
        float *out = a.audio + (srow * a.max_batch + f) * h;
        int s_nan = 0;
        for (int j = tid; j < h; j += NT) {
            const float prev = (g < 0) ? st.rp_old[j] : yp[(size_t)g * n + h + j].x;
            const float v = y[j].x + prev;  // dsp_add_float :171
            out[j] = v;
            if (isnan(v)) s_nan = 1;
        }
        const int dropped = __any(s_nan);
        if (tid == 0) a.nan_flags[srow * a.max_batch + f] = dropped ? 1 : 0;
        if (!dropped) g = f;
    }
    for (int j = tid; j < h; j += NT) st.rp_new[j] = (g < 0) ? st.rp_old[j] : yp[(size_t)g * n + h + j].x;  // :273-275
}

// ---- transform + overlap-add + demodulation in ONE kernel (compile-time plans) -------------------------------
// One wave walks a CHAIN of K consecutive frames of one client: the second half of frame f-1's transform stays in
// registers until frame f adds it (src/signal.cpp:171-172, 235-237), so the n complex values per item that
// k_demod_idft_fixed writes for k_demod_ola to read back (2.9 KB at n = 360: 190 MB per step at 256 clients x 256
// frames) never leave the CU, and k_demod_ola's three dependent round trips per wave disappear with it.  A chain
// that does not start the batch first repeats the transform of the frame before it (FM: of the two frames before
// it - its first sample needs B'_{f0-1}[h-1] = y_{f0-1}[h-1] + y_{f0-2}[n-1]) as warm-up: 1 or 2 transforms more per K.
// Same operations in the same order as the two-kernel path (explicit __fmul_rn / __fadd_rn where the fused form
// would otherwise let the compiler contract what used to be split across two kernels): bit-identical outputs.
//   grid = ceil(nact * ceil(nframes / K) / W), W = blockDim.x / 64; dynamic LDS = (1 + W) * N * 8 bytes

template <int N, int R0, int R1, int R2>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_fixed(DemodArgs a, int nact, int K) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int h = N / 2, NH = (h + 63) / 64;
    const int lane_ = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    const int F = a.nframes;
    int ci, f0, f1;
    if (!wave_chain(nact, F, K, ci, f0, f1)) return;
    ClientParams cp = a.clients[ci];
    // replay (DemodArgs::ssb_mark): the whole batch as ONE chain (K >= F: no warm-up frame, every decision in frame order),
    // for the USB / LSB slots the first launch marked
    if (a.replay && (cp.mode >= 2 || a.ssb_mark[cp.slot] != a.mark_epoch)) return;
    cp = wave_uniform(cp);
    cf *buf = Wn + N + (size_t)wv * N;
    const size_t srow = (size_t)cp.slot;
    const SlotState st = slot_state(a, cp, h);
    const bool ssb = cp.mode < 2;
    cf tail[NH];                         // y_{f-1}[h + j], j = lane + 64 u
    cf blast = make_float2(0.f, 0.f);    // FM: B'_{f-1}[h-1] (wave-uniform)
    // warm-up frames (transformed, nothing written): one before the chain, two for FM; ONE loop body for both kinds
    // of frame (three inlined copies of the transform cost 100 VGPRs more)
    const int fs = f0 == 0 ? 0 : (f0 - (cp.mode == 3 ? 2 : 1) > 0 ? f0 - (cp.mode == 3 ? 2 : 1) : 0);
#pragma unroll
    for (int u = 0; u < NH; u++) {
        const int j = lane_ + 64 * u;
        tail[u] = make_float2(0.f, 0.f);
        // the batch's first frame: the carried state (src/signal.h:86-101)
        if (fs == 0 && j < h) tail[u] = ssb ? make_float2(st.rp_old[j], 0.f) : st.bt_old[j];
    }
    if (fs == 0 && cp.mode == 3) blast = a.bb_last[st.row_old];
    int bad = 0;  // USB / LSB: a non-finite value seen (per lane)
    if (ssb) {
#pragma unroll
        for (int u = 0; u < NH; u++) bad |= not_finite(tail[u].x) ? 1 : 0;
    }
    int f = fs;
    // PSDR_DEMOD_PREFETCH=1: the slice of the NEXT frame is fetched while this frame is transformed (a wave that walks its
    // chain frame by frame has one frame's loads in flight at a time).  Measured on the round-4 build, same box, three
    // interleaved repetitions: 256 clients on cfg2's stream 94.75-94.79 GS/s with it, 94.65-95.06 without; cfg3 and the
    // cfg5 share inside their spread; n = 720 with it (=2: 128 VGPRs + 48 bytes of scratch) -1 %.  The chain kernel's time
    // beside the passes is not its own latency (docs/history.md 5.4): off.
#ifndef PSDR_DEMOD_PREFETCH
#define PSDR_DEMOD_PREFETCH 0
#endif
    constexpr int NR = (N + 63) / 64;
    cf svn[NR];
    int fpre = -1;  // frame whose slice svn holds
    constexpr int HO = NR < 3 ? NR : (N <= 512 ? 3 : 6);
    unsigned so[HO];  // where the slice's first 64 HO bins sit inside a frame: the same for every frame of the chain
    idft_slice_offsets<N, HO>(a, cp, lane_, so);
    const Notches nz = notch_load(a, cp.slot);
    while (f < f1) {
        const bool emit = f >= f0;
        const int lane = opaque_lane(lane_);
        float pw;
        if (PSDR_DEMOD_PREFETCH && (N <= 512 || PSDR_DEMOD_PREFETCH > 1)) {  // (n = 720: 128 VGPRs + 48 bytes of scratch with it)
            cf sv[NR];
            if (f == fpre) {
#pragma unroll
                for (int u = 0; u < NR; u++) sv[u] = svn[u];
            } else {
                idft_load_slice_at<N, HO>(a, cp, nz, f, so, lane, sv);  // the chain's first frame; a warm-up frame looked for further back
            }
            if (f + 1 < f1) {
                idft_load_slice_at<N, HO>(a, cp, nz, f + 1, so, lane, svn);
                fpre = f + 1;
            }
            pw = idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
        } else {
            cf sv[NR];  // loads first, LDS after
            idft_load_slice_at<N, HO>(a, cp, nz, f, so, lane, sv);
            pw = idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
        }
        if (emit && lane == 0) a.pwr[srow * a.max_batch + f] = pw;
        const float sg = frame_sign(a, cp, f);
        float *out = a.audio + (srow * a.max_batch + f) * h;
        const bool last = (f == F - 1);
        int s_nan = 0;
        cf carry = blast;  // FM: b of sample j-1 for the lane that holds j = 64 u (lane 0)
        // y_f[j] and y_f[h + j] of the two-kernel path: the transform output after reversal (LSB) and sign flip.
        // (mode is a scalar: one plain loop per mode - the three-way select inside one unrolled loop is miscompiled
        // by this toolchain, see k_demod_idft_fixed)
        cf yv[NH], yn[NH];
        if (cp.mode == 0) {
#pragma unroll
            for (int u = 0; u < NH; u++) {
                const int j = lane + 64 * u;
                yv[u] = yn[u] = make_float2(0.f, 0.f);
                if (j < h) {
                    yv[u].x = __fmul_rn(buf[j].x, sg);
                    yn[u].x = __fmul_rn(buf[h + j].x, sg);
                }
            }
        } else if (cp.mode == 1) {
#pragma unroll
            for (int u = 0; u < NH; u++) {
                const int j = lane + 64 * u;
                yv[u] = yn[u] = make_float2(0.f, 0.f);
                if (j < h) {
                    yv[u].x = __fmul_rn(buf[N - 1 - j].x, sg);  // std::reverse :155
                    yn[u].x = __fmul_rn(buf[N - 1 - h - j].x, sg);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < NH; u++) {
                const int j = lane + 64 * u;
                yv[u] = yn[u] = make_float2(0.f, 0.f);
                if (j < h) {
                    const cf v0 = buf[j], v1 = buf[h + j];
                    yv[u] = make_float2(__fmul_rn(v0.x, sg), __fmul_rn(v0.y, sg));
                    yn[u] = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NH; u++) {
            const int j = lane + 64 * u;
            const bool ok = j < h;
            const cf y = yv[u], ynext = yn[u];
            float v = 0.f;
            cf b = make_float2(0.f, 0.f);
            if (ssb) {
                v = __fadd_rn(y.x, tail[u].x);  // dsp_add_float :171
            } else {
                b = make_float2(__fadd_rn(y.x, tail[u].x), __fadd_rn(y.y, tail[u].y));  // dsp_add_complex :235
                if (cp.mode == 2) {
                    v = sqrtf(fmaf(b.x, b.x, b.y * b.y));  // dsp_am_demod
                } else {
                    // previous sample: lane-1 of this round; lane 0 takes the last sample of the round before
                    cf pr = make_float2(__shfl_up(b.x, 1, 64), __shfl_up(b.y, 1, 64));
                    if (lane == 0) pr = carry;
                    // arg(b * conj(pr)), src/utils/dsp.cpp:32
                    const float re = fmaf(b.x, pr.x, b.y * pr.y);
                    const float im = fmaf(b.x, -pr.y, b.y * pr.x);
                    v = atan2f(im, re);
                    carry = make_float2(__shfl(b.x, 63, 64), __shfl(b.y, 63, 64));
                    if (u == (h - 1) / 64) blast = make_float2(__shfl(b.x, (h - 1) & 63, 64), __shfl(b.y, (h - 1) & 63, 64));
                }
            }
            if (ok && isnan(v)) s_nan = 1;
            if (ok && emit) {
                out[j] = v;
                if (last && !ssb) {  // the state the next batch starts from (:200-203); the other mode family's is kept
                    st.bt_new[j] = ynext;
                    st.rp_new[j] = st.rp_old[j];
                    if (j == h - 1) a.bb_last[st.row_new] = b;
                }
            }
            if (!ssb) tail[u] = ynext;  // (:200-203 precede the NaN guard: the complex modes' state always moves)
        }
        const int any_nan = __any(s_nan);
        if (ssb) {
#pragma unroll
            for (int u = 0; u < NH; u++) bad |= (not_finite(yv[u].x) || not_finite(yn[u].x)) ? 1 : 0;
            // A dropped USB / LSB frame throws at src/signal.cpp:266-271, BEFORE audio_real_prev is replaced (:273-275):
            // the next frame adds the tail of the latest frame that survived.  (With finite values nothing is dropped; a
            // NaN input sample makes a transform NaN throughout, so for a warm-up frame - whose own tail is unknown here -
            // "y + 0 has a NaN" says the same; any other non-finite value marks the slot for the sequential replay.)
            if (!emit) {
                // the warm-up frame of a chain that does not start the batch: if it was dropped, look further back
                if (any_nan && f > 0) {
                    f--;
                    wave_lds_sync();
                    continue;
                }
#pragma unroll
                for (int u = 0; u < NH; u++) {
                    const int j = lane + 64 * u;
                    tail[u] = yn[u];
                    if (any_nan && j < h) tail[u] = make_float2(st.rp_old[j], 0.f);  // nothing survived before the chain: the carried tail
                }
                f = f0;
                wave_lds_sync();
                continue;
            }
#pragma unroll
            for (int u = 0; u < NH; u++) {
                const int j = lane + 64 * u;
                if (!any_nan) tail[u] = yn[u];
                if (last && j < h) {  // :273-275
                    st.rp_new[j] = tail[u].x;
                    st.bt_new[j] = st.bt_old[j];
                }
            }
            if (last && lane == 0) a.bb_last[st.row_new] = a.bb_last[st.row_old];
        }
        if (emit && lane == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
        wave_lds_sync();  // buf is read out: the next frame's transform may overwrite it
        f++;
    }
    if (ssb && !a.replay && __any(bad) && lane_ == 0) a.ssb_mark[srow] = a.mark_epoch;
}

// ---- PSDR_IQ: the overlap-added complex baseband itself as the client's output ------------------------------------
// IQ_f[j] = s_f y_f[j] + s_{f-1} y_{f-1}[h + j], j < h: what AM and FM hold in `b` above before sqrtf / atan2f collapse it
// (audio_complex_baseband after src/signal.cpp:235-237), stored as (re, im) rows iq[slot][max_batch][h].  IQ clients are
// listed apart (a.clients = their list, nact = their number) and served by these two kernels alone; the transform is the
// AM / FM one (every IDFT kernel above treats mode >= 2 as a complex transform into ypost).  The carried state is AM's
// and FM's - bb_tail, bb_last = IQ_f[h-1], real_prev copied through - and always moves; the NaN flag of a frame is 1
// if any component of IQ_f is NaN.

// n = 360 / 720: one wave per chain of K frames of an IQ client, the tail in registers - the shared steps of
// k_demod_chain_fixed (stage_twiddles, wave_chain, wave_uniform, slot_state, frame_sign, opaque_lane) around its own frame body:
// ONE warm-up frame (no sample of IQ_f0 looks further back than y_{f0-1}), no detector, no NaN-guard replay, no
// ssb_mark.  Same operations in the same order as k_demod_idft_fixed + k_demod_ola_iq (__fmul_rn / __fadd_rn: see
// k_demod_chain_fixed): bit-identical outputs.  Grid and LDS as k_demod_chain_fixed.
// NZ: the notch test (notched, above) is part of the slice load.  Beside a pass k_demod_chain_iq<360> holds 62 VGPRs and 102
// scalar registers; with the test in, every form tried took 65 - 67 (scalars spilled into vector lanes).  So the kernel
// without the test stays what it was, and k_demod_chain_iq_nz - the same body, NZ = true - serves the IQ lists that contain
// a notched client.
template <int N, int R0, int R1, int R2, bool NZ>
__device__ __forceinline__ void demod_chain_iq_body(const DemodArgs &a, int nact, int K, cf *iq) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int h = N / 2, NH = (h + 63) / 64;
    const int lane_ = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    const int F = a.nframes;
    int ci, f0, f1;
    if (!wave_chain(nact, F, K, ci, f0, f1)) return;
    const ClientParams cp = wave_uniform(a.clients[ci]);
    cf *buf = Wn + N + (size_t)wv * N;
    const size_t srow = (size_t)cp.slot;
    const SlotState st = slot_state(a, cp, h);
    const int fs = f0 == 0 ? 0 : f0 - 1;  // the warm-up frame: transformed, nothing written
    cf tail[NH];                          // s_{f-1} y_{f-1}[h + j], j = lane + 64 u
#pragma unroll
    for (int u = 0; u < NH; u++) {
        const int j = lane_ + 64 * u;
        tail[u] = make_float2(0.f, 0.f);
        if (fs == 0 && j < h) tail[u] = st.bt_old[j];  // the batch's first frame: the carried tail
    }
    constexpr int NR = (N + 63) / 64;
    constexpr int HO = NR < 3 ? NR : (N <= 512 ? 3 : 6);
    unsigned so[HO];
    idft_slice_offsets<N, HO>(a, cp, lane_, so);
    for (int f = fs; f < f1; f++) {
        const bool emit = f >= f0;
        const int lane = opaque_lane(lane_);
        Notches nz{};
        if constexpr (NZ) nz = notch_load_frame(a, cp.slot);
        cf sv[NR];  // loads first, LDS after
        idft_load_slice_at<N, HO, NZ>(a, cp, nz, f, so, lane, sv);
        const float pw = idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
        if (emit && lane == 0) a.pwr[srow * a.max_batch + f] = pw;
        const float sg = frame_sign(a, cp, f);
        cf *out = iq + (srow * a.max_batch + f) * h;
        const bool last = (f == F - 1);
        int s_nan = 0;
#pragma unroll
        for (int u = 0; u < NH; u++) {
            const int j = lane + 64 * u;
            if (j < h) {
                const cf v0 = buf[j], v1 = buf[h + j];
                const cf y = make_float2(__fmul_rn(v0.x, sg), __fmul_rn(v0.y, sg));
                const cf ynext = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                const cf b = make_float2(__fadd_rn(y.x, tail[u].x), __fadd_rn(y.y, tail[u].y));  // dsp_add_complex :235
                if (isnan(b.x) || isnan(b.y)) s_nan = 1;
                if (emit) {
                    out[j] = b;
                    if (last) {  // the state the next batch starts from (:200-203); USB / LSB's is kept
                        st.bt_new[j] = ynext;
                        st.rp_new[j] = st.rp_old[j];
                        if (j == h - 1) a.bb_last[st.row_new] = b;
                    }
                }
                tail[u] = ynext;
            }
        }
        const int any_nan = __any(s_nan);
        if (emit && lane == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
        wave_lds_sync();  // buf is read out: the next frame's transform may overwrite it
    }
}
template <int N, int R0, int R1, int R2>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_iq(DemodArgs a, int nact, int K, cf *iq) {
    demod_chain_iq_body<N, R0, R1, R2, false>(a, nact, K, iq);
}
template <int N, int R0, int R1, int R2>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_iq_nz(DemodArgs a, int nact, int K, cf *iq) {
    demod_chain_iq_body<N, R0, R1, R2, true>(a, nact, K, iq);
}

// any other n (and n = 360 / 720 with PSDR_DEMOD_CHAIN=0): the overlap-add of an IQ client's rows of ypost, beside
// k_demod_ola and with its grid - one wave per (client, group of PSDR_OLA_FG frames)
__global__ __launch_bounds__(256) void k_demod_ola_iq(DemodArgs a, int nact, cf *iq) {
    constexpr int FG = PSDR_OLA_FG;
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int F = a.nframes, ngrp = (F + FG - 1) / FG;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nact * ngrp) return;
    const int ci = item / ngrp;
    const ClientParams cp = a.clients[ci];
    const int f0 = (item - ci * ngrp) * FG;
    const size_t srow = (size_t)cp.slot;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;  // this client's frames
    const SlotState st = slot_state(a, cp, h);
#pragma unroll
    for (int g = 0; g < FG; g++) {
        const int f = f0 + g;
        if (f >= F) break;
        cf *out = iq + (srow * a.max_batch + f) * h;
        int s_nan = 0;
        for (int j = tid; j < h; j += NT)
            ola_step(a, st, yp, f, j, [&](cf b) {
                out[j] = b;
                if (isnan(b.x) || isnan(b.y)) s_nan = 1;
            });
        const int any_nan = __any(s_nan);
        if (tid == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
    }
}

// ---- PSDR_SAM: synchronous AM, the baseband detected against the recovered carrier -------------------------------
// The reference's HAS_LIQUID branch (src/signal.cpp:205-222, 230-233, 238-252) transforms the placed bins a second time
// with the indices [cutoff, n - cutoff) zeroed (cutoff = 500 n / audio_rate: a +-500 Hz low-pass around bin
// floor(audio_mid)), overlap-adds that "carrier" baseband C with a tail of its own and feeds B and C to liquid's PLL.  Here
// C is the phase reference itself, feed-forward:
//   audio_f[j] = (B.re C.re + B.im C.im) / |C|   (|C| == 0: B.re),  B = the PSDR_IQ row, C_f[j] = s_f c_f[j] + s_{f-1} c_{f-1}[h + j]
// every operation correctly rounded and in a fixed order (sam_detect), so no batch split changes a bit.  SAM clients are
// listed apart (a.clients = their list, nact = their number), like IQ clients.  State: bb_tail / bb_last / real_prev as
// AM, plus the carrier tail s_f c_f[h..n) in SamArgs::car_tail [2][slots][h]; the host zeroes the current half for a slot
// whose previous batch was not SAM.  Per frame one carrier record (level, offset_hz) in car_rec[slot][max_batch]:
//   level = mean_j |C[j]|,  offset_hz = hz_per_rad * arg( sum_{1 <= j < h} C[j] conj(C[j-1]) )
struct SamArgs {
    cf *car_tail;      // [2][slots][n/2]
    cf *car_rec;       // [slots][max_batch] (level, offset_hz)
    int cutoff;        // placed indices [cutoff, n - cutoff) are zeroed: slice bin t is kept iff -cutoff <= t - m < cutoff
    float hz_per_rad;  // audio_rate / (2 pi)
};
__device__ __forceinline__ float sam_detect(cf b, cf c, float &mag) {
    mag = __fsqrt_rn(__fadd_rn(__fmul_rn(c.x, c.x), __fmul_rn(c.y, c.y)));
    const float num = __fadd_rn(__fmul_rn(b.x, c.x), __fmul_rn(b.y, c.y));
    return mag == 0.f ? b.x : __fdiv_rn(num, mag);
}
// one term of the offset sum: c conj(p)
__device__ __forceinline__ cf sam_lag(cf c, cf p) {
    return make_float2(fmaf(c.x, p.x, c.y * p.y), fmaf(c.y, p.x, -(c.x * p.y)));
}
// n = 360 / 720: the same shared steps as k_demod_chain_iq - one wave per chain of K frames, ONE warm-up frame, both tails
// (B's and C's) in registers.  Per frame the compile-time plan runs twice through ONE loop body (two inlined copies would double the code
// and the address registers): pass 0 on the masked slice gives c_f, pass 1 on the whole slice gives y_f exactly as
// k_demod_chain_iq computes it (B is bit-identical to the PSDR_IQ rows).  The second plan run instead of a direct sum over
// the 2 cutoff kept bins: at n = 360 and 12 kHz the direct sum is 30 bins x 6 outputs per lane = 180 complex MACs (720 FMAs
// and as many twiddle look-ups with an index product modulo n), the plan ~250 packed instructions with base + immediate
// addressing; at n = 720 it is 2880 FMAs against ~600.  The slice is loaded again for pass 1 (L1 / L2 hits) instead of
// being held in 2 NR registers across pass 0.  Grid as k_demod_chain_fixed; dynamic LDS = ((1 + W) * N + W * N/2) * 8 bytes.
template <int N, int R0, int R1, int R2>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_sam(DemodArgs a, int nact, int K, SamArgs sa) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int h = N / 2, NH = (h + 63) / 64;
    const int lane_ = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    const int F = a.nframes;
    int ci, f0, f1;
    if (!wave_chain(nact, F, K, ci, f0, f1)) return;
    const ClientParams cp = wave_uniform(a.clients[ci]);
    cf *buf = Wn + N + (size_t)wv * N;
    const size_t srow = (size_t)cp.slot;
    const SlotState st = slot_state(a, cp, h);
    const cf *ct_old = sa.car_tail + st.row_old * h;
    cf *ct_new = sa.car_tail + st.row_new * h;
    const int fs = f0 == 0 ? 0 : f0 - 1;  // the warm-up frame: transformed, nothing written
    cf tail[NH];                          // s_{f-1} y_{f-1}[h + j], j = lane + 64 u
    // ... and s_{f-1} c_{f-1}[h + j] in h words of LDS of the wave's own behind the transform buffers: entry j is read and
    // written by the lane that owns j alone (no wait between lanes), once per frame
    cf *ctail = Wn + N + (size_t)W * N + (size_t)wv * h;
#pragma unroll
    for (int u = 0; u < NH; u++) {
        const int j = lane_ + 64 * u;
        tail[u] = make_float2(0.f, 0.f);
        if (j < h) {
            ctail[j] = make_float2(0.f, 0.f);
            if (fs == 0) tail[u] = st.bt_old[j], ctail[j] = ct_old[j];  // the batch's first frame: the carried tails
        }
    }
    constexpr int NR = (N + 63) / 64;
    constexpr int HO = NR < 3 ? NR : (N <= 512 ? 3 : 2);  // (n = 720: the registers of four more offsets are the difference to scratch)
    unsigned so[HO];
    idft_slice_offsets<N, HO>(a, cp, lane_, so);
    const int m = cp.m_floor - cp.l;
    cf cC[NH];  // C_f[j], from pass 0 of a frame to its pass 1
#pragma unroll
    for (int u = 0; u < NH; u++) cC[u] = make_float2(0.f, 0.f);
    // ONE loop over (frame, pass): a single copy of the transform in the kernel, as in k_demod_chain_iq
    for (int it = 2 * fs; it < 2 * f1; it++) {
        const int f = it >> 1, pass = it & 1;
        const bool emit = f >= f0;
        const float sg = frame_sign(a, cp, f);
        float *out = a.audio + (srow * a.max_batch + f) * h;
        const bool last = (f == F - 1);
        {
            const int lane = opaque_lane(lane_);
            const Notches nz = notch_load_frame(a, cp.slot);
            cf sv[NR];  // loads first, LDS after
            idft_load_slice_at<N, HO>(a, cp, nz, f, so, lane, sv);
            if (pass == 0) {
#pragma unroll
                for (int u = 0; u < NR; u++) {
                    const int d = lane + 64 * u - m;
                    if (d < -sa.cutoff || d >= sa.cutoff) sv[u] = make_float2(0.f, 0.f);
                }
            }
            const float pw = idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
            if (pass == 0) {
#pragma unroll
                for (int u = 0; u < NH; u++) {
                    const int j = lane + 64 * u;
                    cC[u] = make_float2(0.f, 0.f);
                    if (j < h) {
                        const cf v0 = buf[j], v1 = buf[h + j];
                        const cf ct = ctail[j];
                        cC[u] = make_float2(__fadd_rn(__fmul_rn(v0.x, sg), ct.x), __fadd_rn(__fmul_rn(v0.y, sg), ct.y));
                        ctail[j] = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                    }
                }
            } else {
                if (emit && lane == 0) a.pwr[srow * a.max_batch + f] = pw;
                int s_nan = 0;
                float lvl = 0.f;
                cf lag = make_float2(0.f, 0.f), ccarry = make_float2(0.f, 0.f);
#pragma unroll
                for (int u = 0; u < NH; u++) {
                    const int j = lane + 64 * u;
                    const cf c = cC[u];
                    cf pr = make_float2(__shfl_up(c.x, 1, 64), __shfl_up(c.y, 1, 64));  // C[j-1]
                    if (lane == 0) pr = ccarry;
                    ccarry = make_float2(__shfl(c.x, 63, 64), __shfl(c.y, 63, 64));
                    if (j < h) {
                        const cf v0 = buf[j], v1 = buf[h + j];
                        const cf y = make_float2(__fmul_rn(v0.x, sg), __fmul_rn(v0.y, sg));
                        const cf ynext = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                        const cf b = make_float2(__fadd_rn(y.x, tail[u].x), __fadd_rn(y.y, tail[u].y));  // dsp_add_complex :235
                        float mag;
                        const float v = sam_detect(b, c, mag);
                        if (isnan(v)) s_nan = 1;
                        lvl += mag;
                        if (j > 0) {
                            const cf t = sam_lag(c, pr);
                            lag.x += t.x, lag.y += t.y;
                        }
                        if (emit) {
                            out[j] = v;
                            if (last) {  // the state the next batch starts from (:200-203 precede the NaN guard); USB / LSB's is kept
                                st.bt_new[j] = ynext;
                                ct_new[j] = ctail[j];
                                st.rp_new[j] = st.rp_old[j];
                                if (j == h - 1) a.bb_last[st.row_new] = b;
                            }
                        }
                        tail[u] = ynext;
                    }
                }
                const int any_nan = __any(s_nan);
                lvl = wave_sum(lvl);
                lag.x = wave_sum(lag.x), lag.y = wave_sum(lag.y);
                if (emit && lane == 0) {
                    a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
                    sa.car_rec[srow * a.max_batch + f] = make_float2(lvl / (float)h, sa.hz_per_rad * atan2f(lag.y, lag.x));
                }
            }
            wave_lds_sync();  // buf is read out: the next transform may overwrite it
        }
    }
}

// c_f[jout] of a SAM client by the direct sum over its kept bins d = t - m in [d0, d1), read from the spectrum:
//   sum_d X[m_floor + d] W_n^{(d mod n) jout}
__device__ __forceinline__ cf sam_carrier_dsum(const DemodArgs &a, const ClientParams &cp, const Notches &nz, const cf *S, int d0, int d1, int jout) {
    const unsigned n = (unsigned)a.n;
    float ar = 0.f, ai = 0.f;
    for (int d = d0; d < d1; d++) {
        const cf x = notched(nz, cp, cp.m_floor + d - cp.l) ? make_float2(0.f, 0.f) : S[a.lay.pos(cp.m_floor + d)];
        const cf w = a.Wn[((unsigned)(d < 0 ? (int)n + d : d) * (unsigned)jout) % n];  // (< n^2 < 2^32: demodplan.h sam_size_served, no client becomes PSDR_SAM at n >= 2^16)
        ar = fmaf(x.x, w.x, fmaf(-x.y, w.y, ar));
        ai = fmaf(x.x, w.y, fmaf(x.y, w.x, ai));
    }
    return make_float2(ar, ai);
}

// any other n (and n = 360 / 720 with PSDR_DEMOD_CHAIN=0): behind the IDFT kernels, with k_demod_ola_iq's grid - one wave
// per (client, group of PSDR_OLA_FG frames).  B from the client's rows of ypost exactly as k_demod_ola_iq adds them; the
// carrier by the direct sum above (no second ypost): c_f[j], c_{f-1}[h + j] (the batch's first frame: the carried tail)
// and, for the batch's last frame, c_f[h + j] for the tail.  The same function wherever a value is needed: the bits do
// not depend on the batch split or on the frame's place in its group.
__global__ __launch_bounds__(256) void k_demod_ola_sam(DemodArgs a, int nact, SamArgs sa) {
    constexpr int FG = PSDR_OLA_FG;
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int F = a.nframes, ngrp = (F + FG - 1) / FG;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nact * ngrp) return;
    const int ci = item / ngrp;
    const ClientParams cp = a.clients[ci];
    const int f0 = (item - ci * ngrp) * FG;
    const size_t srow = (size_t)cp.slot;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;  // this client's frames
    const SlotState st = slot_state(a, cp, h);
    const cf *ct_old = sa.car_tail + st.row_old * h;
    cf *ct_new = sa.car_tail + st.row_new * h;
    const Notches nz = notch_load(a, cp.slot);
    // kept AND placed AND inside the slice: d = t - m with 0 <= t < r - l, -(h - 1) <= d < h, -cutoff <= d < cutoff
    const int m = cp.m_floor - cp.l, len = cp.r - cp.l;
    int d0 = -sa.cutoff, d1 = sa.cutoff;
    if (d0 < -(h - 1)) d0 = -(h - 1);
    if (d0 < -m) d0 = -m;
    if (d1 > h) d1 = h;
    if (d1 > len - m) d1 = len - m;
    for (int g = 0; g < FG; g++) {
        const int f = f0 + g;
        if (f >= F) break;
        const cf *S = a.spec + (size_t)f * a.spec_stride;
        const float sg = frame_sign(a, cp, f), sgp = frame_sign(a, cp, f - 1);
        float *out = a.audio + (srow * a.max_batch + f) * h;
        int s_nan = 0;
        const bool last = (f == F - 1);
        float lvl = 0.f;
        cf lag = make_float2(0.f, 0.f), ccarry = make_float2(0.f, 0.f);
        for (int j0 = 0; j0 < h; j0 += NT) {  // (every lane walks every round: the shuffles below need the whole wave)
            const int j = j0 + tid;
            const bool ok = j < h;
            cf c = make_float2(0.f, 0.f);
            if (ok) {
                const cf cy = sam_carrier_dsum(a, cp, nz, S, d0, d1, j);
                cf ct;
                if (f == 0) {
                    ct = ct_old[j];
                } else {
                    const cf cp1 = sam_carrier_dsum(a, cp, nz, S - a.spec_stride, d0, d1, h + j);
                    ct = make_float2(__fmul_rn(cp1.x, sgp), __fmul_rn(cp1.y, sgp));
                }
                c = make_float2(__fadd_rn(__fmul_rn(cy.x, sg), ct.x), __fadd_rn(__fmul_rn(cy.y, sg), ct.y));
            }
            cf pr = make_float2(__shfl_up(c.x, 1, 64), __shfl_up(c.y, 1, 64));  // C[j-1]
            if (tid == 0) pr = ccarry;
            ccarry = make_float2(__shfl(c.x, 63, 64), __shfl(c.y, 63, 64));
            if (ok)
                ola_step(a, st, yp, f, j, [&](cf b) {
                    float mag;
                    const float v = sam_detect(b, c, mag);
                    out[j] = v;
                    if (isnan(v)) s_nan = 1;
                    lvl += mag;
                    if (j > 0) {
                        const cf t = sam_lag(c, pr);
                        lag.x += t.x, lag.y += t.y;
                    }
                    if (last) {  // the carrier's tail moves with the baseband's
                        const cf cn = sam_carrier_dsum(a, cp, nz, S, d0, d1, h + j);
                        ct_new[j] = make_float2(__fmul_rn(cn.x, sg), __fmul_rn(cn.y, sg));
                    }
                });
        }
        const int any_nan = __any(s_nan);
        lvl = wave_sum(lvl);
        lag.x = wave_sum(lag.x), lag.y = wave_sum(lag.y);
        if (tid == 0) {
            a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
            sa.car_rec[srow * a.max_batch + f] = make_float2(lvl / (float)h, sa.hz_per_rad * atan2f(lag.y, lag.x));
        }
    }
}

// ---- fine tuning below one FFT bin: USB / LSB / IQ clients with the fine-tune flag (include/psdr.h) --------------------
// The bins are placed around m = floor(audio_mid) as ever; the fraction delta = audio_mid - m is taken out behind the
// overlap-add by a rotator at the audio rate, w(phi) = exp(-2 pi i phi / 2^32), phi_{f,j} = phi0 + (f h + j) step in wrapping
// 32-bit arithmetic (step = round(delta 2^32 / n); the host carries phi0 from batch to batch):
//   tuned IQ        row_f[j]   = B_f[j] w(phi_{f,j}),         B  = the PSDR_IQ row of the window
//   tuned USB / LSB audio_f[j] = 2 Re(B'_f[j] w(phi_{f,j})),  B' = the PSDR_IQ row of the window CLIPPED to the sideband
// Tuned clients are listed apart: a.clients[ci] carries the PLACED range [l, r) (the clipped window; the whole one for IQ)
// with the AM / FM placement as its mode - the list every IDFT kernel above takes as it is - and FtArgs::ft[ci] (FtClient, types.h) the phase,
// the step and the WHOLE window, over which pwr is summed.  One launch serves one family (SSB: float rows of `audio`, a tail
// of its own in FtArgs::tail, every other piece of state copied through; IQ: complex rows of `iq`, IQ's state).
struct FtArgs {
    const FtClient *ft;  // [nact], beside a.clients
    cf *tail;            // SSB: [2][slots][n/2], s_f y'_f[h..n) of the clipped transform
    cf *iq;              // IQ: the rows [slots][max_batch][n/2]
};
__device__ __forceinline__ cf ft_cmul(cf a, cf b) {
    return make_float2(__fmaf_rn(a.x, b.x, -__fmul_rn(a.y, b.y)), __fmaf_rn(a.x, b.y, __fmul_rn(a.y, b.x)));
}
// w(phi): the nearest quarter turn q comes off in integers, the rest r (|r| <= 2^29 units = an eighth of a turn) goes
// through the degree-7 / degree-8 polynomials of sin and cos on [-pi/4, pi/4] (Cephes sinf / cosf: below 1 ulp of 1 there).
// int -> float rounds r to 24 bits, 2^-28 turn.
__device__ __forceinline__ cf ft_rot(unsigned phi) {
    const unsigned q = (phi + 0x20000000u) >> 30;
    const int r = (int)(phi - (q << 30));
    const float x = __fmul_rn(__int2float_rn(r), 1.4629180792671596e-9f);  // 2 pi / 2^32
    const float z = __fmul_rn(x, x);
    const float ps = __fmaf_rn(__fmaf_rn(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float pc = __fmaf_rn(__fmaf_rn(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float s = __fmaf_rn(__fmul_rn(x, z), ps, x);
    const float c = __fmaf_rn(__fmul_rn(z, z), pc, __fmaf_rn(z, -0.5f, 1.f));
    // theta = q pi/2 + x: (cos, sin) = (c, s), (-s, c), (-c, -s), (s, -c) for q = 0 .. 3; w = (cos theta, -sin theta)
    const float co = (q & 1u) ? s : c, si = (q & 1u) ? c : s;
    return make_float2(((q + 1u) & 2u) ? -co : co, (q & 2u) ? si : -si);
}
// The rotators of a frame for the samples j0 + 64 u of one lane, phl = the phase of sample j0.  Two forms, both pure
// functions of (phl, step, u): the direct one evaluates w at every sample's phase; the product one evaluates it at the
// lane's first sample and multiplies with the wave-uniform constant w(64 u step), which a chain kernel computes once per
// chain.  The same form in every kernel (DESIGN.md 3.9 has the instruction counts that chose it).
#ifndef PSDR_FT_ROTATOR_DIRECT
#define PSDR_FT_ROTATOR_DIRECT 0
#endif
__device__ __forceinline__ cf ft_w(unsigned phl, unsigned step, int u) {
    if (PSDR_FT_ROTATOR_DIRECT || u == 0) return ft_rot(phl + 64u * (unsigned)u * step);
    return ft_cmul(ft_rot(phl), ft_rot(64u * (unsigned)u * step));
}

// n = 360 / 720: the sibling of k_demod_chain_iq - one wave per chain of K frames, ONE warm-up frame, the tail in registers,
// the same shared steps.  The slice is loaded over the whole window, summed for pwr exactly as idft_slice_fixed sums it, and
// the bins outside the placed range are zeroed before the scatter: the buffer the stages see is the one a PSDR_IQ client on
// the clipped window gives them, so B' is bit-identical to that client's rows.  SSB is a template flag: nothing in the frame
// loop branches on the family.  Grid and LDS as k_demod_chain_iq.
template <int N, int R0, int R1, int R2, bool SSB>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_ft(DemodArgs a, int nact, int K, FtArgs fa) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int h = N / 2, NH = (h + 63) / 64;
    const int lane_ = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    const int F = a.nframes;
    int ci, f0, f1;
    if (!wave_chain(nact, F, K, ci, f0, f1)) return;
    const ClientParams cp = wave_uniform(a.clients[ci]);  // [l, r): the placed range
    FtClient fc = fa.ft[ci];
    fc.phi0 = __builtin_amdgcn_readfirstlane(fc.phi0);
    fc.step = __builtin_amdgcn_readfirstlane(fc.step);
    fc.l = __builtin_amdgcn_readfirstlane(fc.l);
    fc.r = __builtin_amdgcn_readfirstlane(fc.r);
    ClientParams cw = cp;  // the whole window: what is loaded and summed
    cw.l = fc.l, cw.r = fc.r;
    const int t0 = cp.l - fc.l, t1 = cp.r - fc.l;  // slice bins [t0, t1) are placed
    cf *buf = Wn + N + (size_t)wv * N;
    const size_t srow = (size_t)cp.slot;
    const SlotState st = slot_state(a, cp, h);
    const cf *tl_old = SSB ? fa.tail + st.row_old * h : st.bt_old;
    cf *tl_new = SSB ? fa.tail + st.row_new * h : st.bt_new;
    const int fs = f0 == 0 ? 0 : f0 - 1;  // the warm-up frame: transformed, nothing written
    cf tail[NH];                          // s_{f-1} y_{f-1}[h + j], j = lane + 64 u
#pragma unroll
    for (int u = 0; u < NH; u++) {
        const int j = lane_ + 64 * u;
        tail[u] = make_float2(0.f, 0.f);
        if (fs == 0 && j < h) tail[u] = tl_old[j];  // the batch's first frame: the carried tail
    }
#if !PSDR_FT_ROTATOR_DIRECT
    cf wu[NH];  // w(64 u step): wave-uniform, in scalar registers (the bits are ft_w's)
#pragma unroll
    for (int u = 1; u < NH; u++) {
        const cf t = ft_rot(64u * (unsigned)u * fc.step);
        wu[u] = make_float2(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.x))),
                            __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.y))));
    }
#endif
    constexpr int NR = (N + 63) / 64;
    constexpr int HO = NR < 3 ? NR : (N <= 512 ? 3 : 6);
    unsigned so[HO];
    idft_slice_offsets<N, HO>(a, cw, lane_, so);
    const Notches nz = notch_load(a, cp.slot);
    for (int f = fs; f < f1; f++) {
        const bool emit = f >= f0;
        const int lane = opaque_lane(lane_);
        cf sv[NR];  // loads first, LDS after
        idft_load_slice_at<N, HO>(a, cw, nz, f, so, lane, sv);
        float pw = 0.f;
#pragma unroll
        for (int u = 0; u < NR; u++) {
            const int t = lane + 64 * u;
            if (t < cw.r - cw.l) pw += fmaf(sv[u].x, sv[u].x, sv[u].y * sv[u].y);  // (idft_slice_fixed's sum, over the whole window)
            if (t < t0 || t >= t1) sv[u] = make_float2(0.f, 0.f);
        }
        pw = wave_sum(pw);
        idft_slice_fixed<N, R0, R1, R2>(cw, sv, buf, Wn, lane);
        if (emit && lane == 0) a.pwr[srow * a.max_batch + f] = pw;
        const float sg = frame_sign(a, cp, f);
        const bool last = (f == F - 1);
        const unsigned phl = fc.phi0 + ((unsigned)f * (unsigned)h + (unsigned)lane) * fc.step;
        const cf w0 = ft_rot(phl);
        int s_nan = 0;
#pragma unroll
        for (int u = 0; u < NH; u++) {
            const int j = lane + 64 * u;
            if (j < h) {
                const cf v0 = buf[j], v1 = buf[h + j];
                const cf y = make_float2(__fmul_rn(v0.x, sg), __fmul_rn(v0.y, sg));
                const cf ynext = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                const cf b = make_float2(__fadd_rn(y.x, tail[u].x), __fadd_rn(y.y, tail[u].y));  // dsp_add_complex :235
#if PSDR_FT_ROTATOR_DIRECT
                const cf w = ft_w(phl, fc.step, u);
#else
                const cf w = u == 0 ? w0 : ft_cmul(w0, wu[u]);
#endif
                if constexpr (SSB) {
                    const float v = __fmul_rn(2.f, __fmaf_rn(b.x, w.x, -__fmul_rn(b.y, w.y)));
                    if (isnan(v)) s_nan = 1;
                    if (emit) {
                        a.audio[(srow * a.max_batch + f) * h + j] = v;
                        if (last) {  // the client's own tail moves; every other mode's state is copied through
                            tl_new[j] = ynext;
                            st.bt_new[j] = st.bt_old[j];
                            st.rp_new[j] = st.rp_old[j];
                            if (j == h - 1) a.bb_last[st.row_new] = a.bb_last[st.row_old];
                        }
                    }
                } else {
                    const cf o = ft_cmul(b, w);
                    if (isnan(o.x) || isnan(o.y)) s_nan = 1;
                    if (emit) {
                        fa.iq[(srow * a.max_batch + f) * h + j] = o;
                        if (last) {  // IQ's state: the UN-rotated baseband's (:200-203); USB / LSB's is kept
                            tl_new[j] = ynext;
                            st.rp_new[j] = st.rp_old[j];
                            if (j == h - 1) a.bb_last[st.row_new] = b;
                        }
                    }
                }
                tail[u] = ynext;
            }
        }
        const int any_nan = __any(s_nan);
        if (emit && lane == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
        wave_lds_sync();  // buf is read out: the next frame's transform may overwrite it
    }
}

// any other n (and n = 360 / 720 with PSDR_DEMOD_CHAIN=0): behind the IDFT kernels on the tuned list, with k_demod_ola_iq's
// grid: ola_step, the shared rotator, a float or a float2 store.  The IDFT kernel summed pwr over the placed range: the
// whole window's sum is written here, in idft_slice_fixed's order (bit-identical to the chain kernel's).
template <bool SSB>
__global__ __launch_bounds__(256) void k_demod_ola_ft(DemodArgs a, int nact, FtArgs fa) {
    constexpr int FG = PSDR_OLA_FG;
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int F = a.nframes, ngrp = (F + FG - 1) / FG;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nact * ngrp) return;
    const int ci = item / ngrp;
    const ClientParams cp = a.clients[ci];
    const FtClient fc = fa.ft[ci];
    ClientParams cw = cp;  // the whole window: pwr's
    cw.l = fc.l, cw.r = fc.r;
    const Notches nz = notch_load(a, cp.slot);
    const int f0 = (item - ci * ngrp) * FG;
    const size_t srow = (size_t)cp.slot;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;  // this client's frames
    const SlotState st = slot_state(a, cp, h);
    SlotState sm = st;  // the tail ola_step adds and moves: the client's own for SSB
    if (SSB) sm.bt_old = fa.tail + st.row_old * h, sm.bt_new = fa.tail + st.row_new * h;
#pragma unroll
    for (int g = 0; g < FG; g++) {
        const int f = f0 + g;
        if (f >= F) break;
        const cf *S = a.spec + (size_t)f * a.spec_stride;
        float pw = 0.f;
        for (int t = tid; t < fc.r - fc.l; t += NT) {
            const cf v = notched(nz, cw, t) ? make_float2(0.f, 0.f) : S[a.lay.pos(fc.l + t)];
            pw += fmaf(v.x, v.x, v.y * v.y);
        }
        pw = wave_sum(pw);
        if (tid == 0) a.pwr[srow * a.max_batch + f] = pw;
        const unsigned phl = fc.phi0 + ((unsigned)f * (unsigned)h + (unsigned)tid) * fc.step;
        int s_nan = 0, u = 0;
        for (int j = tid; j < h; j += NT, u++) {
            ola_step(a, sm, yp, f, j, [&](cf b) {
                const cf w = ft_w(phl, fc.step, u);
                if constexpr (SSB) {
                    const float v = __fmul_rn(2.f, __fmaf_rn(b.x, w.x, -__fmul_rn(b.y, w.y)));
                    a.audio[(srow * a.max_batch + f) * h + j] = v;
                    if (isnan(v)) s_nan = 1;
                } else {
                    const cf o = ft_cmul(b, w);
                    fa.iq[(srow * a.max_batch + f) * h + j] = o;
                    if (isnan(o.x) || isnan(o.y)) s_nan = 1;
                }
            });
            if (SSB && f == F - 1) {  // (ola_step moved the client's own tail as AM's: the AM / FM state is copied through instead)
                st.bt_new[j] = st.bt_old[j];
                if (j == h - 1) a.bb_last[st.row_new] = a.bb_last[st.row_old];
            }
        }
        const int any_nan = __any(s_nan);
        if (tid == 0) a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
    }
}

// ---- selectable-sideband SAM: a PSDR_SAM client with PSDR_SAM_UPPER / PSDR_SAM_LOWER (include/psdr.h) ------------------------
// The carrier C_f is PSDR_SAM's, from the WHOLE window; the baseband B'_f is built from the window clipped to the sideband
// (tuned USB / LSB's clipping rule) with a tail of its own in SbArgs::tail;
//   audio_f[j] = 2 sam_detect(B', C)
// Sideband SAM clients are listed apart, behind SAM's: a.clients[ci] carries the PLACED range [l, r) (the clipped window)
// with the AM / FM placement as its mode - the list every IDFT kernel above takes as it is - and SbArgs::sb[ci] (SbClient,
// types.h) the sideband and the WHOLE window, from which the carrier is built and over which pwr is summed.  The AM / FM
// tail and last sample and the USB / LSB tail are copied through; the carrier tail is SamArgs::car_tail, shared with
// PSDR_SAM_BOTH (a change of sideband does not interrupt it).
// (The bodies are written out beside k_demod_chain_sam / k_demod_ola_sam, not shared with them: those two stay the code
// they were, register for register.)
struct SbArgs {
    SamArgs sa;
    const SbClient *sb;  // [nact], beside a.clients
    cf *tail;            // [2][slots][n/2], s_f y'_f[h..n) of the clipped transform
};
// n = 360 / 720: the sibling of k_demod_chain_sam - one wave per chain of K frames, ONE warm-up frame, B''s tail in
// registers and C's in LDS, one loop over (frame, pass).  cp carries the whole window: pass 0 runs on the carrier-masked
// slice, pass 1 on the slice masked to the sideband (d = t - m >= 0: upper, d <= 0: lower) - the buffer the stages see is the
// one a PSDR_IQ client on the clipped window gives them, so B' is bit-identical to that client's rows.  Both masks are one
// range test [lo, hi) on d.  pwr is summed from the unmasked slice exactly as idft_slice_fixed sums it.  Grid and LDS as
// k_demod_chain_sam.
template <int N, int R0, int R1, int R2>
__global__ __launch_bounds__(256, N <= 512 ? PSDR_IDFT_WPE : PSDR_IDFT_WPE - 1) void k_demod_chain_sbsam(DemodArgs a, int nact, int K, SbArgs sb) {
    static_assert(R0 * R1 * R2 == N, "plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int h = N / 2, NH = (h + 63) / 64;
    const int lane_ = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
    cf *Wn = stage_twiddles(a, smem, N);
    const int F = a.nframes;
    int ci, f0, f1;
    if (!wave_chain(nact, F, K, ci, f0, f1)) return;
    ClientParams cp = a.clients[ci];
    const SbClient sc = sb.sb[ci];
    cp.l = sc.l, cp.r = sc.r;  // the whole window: what is loaded, summed and placed (behind the masks)
    cp = wave_uniform(cp);
    const bool upper = __builtin_amdgcn_readfirstlane(sc.side) == 1;  // PSDR_SAM_UPPER
    cf *buf = Wn + N + (size_t)wv * N;
    const size_t srow = (size_t)cp.slot;
    const SlotState st = slot_state(a, cp, h);
    const cf *ct_old = sb.sa.car_tail + st.row_old * h;
    cf *ct_new = sb.sa.car_tail + st.row_new * h;
    const cf *tl_old = sb.tail + st.row_old * h;
    cf *tl_new = sb.tail + st.row_new * h;
    const int fs = f0 == 0 ? 0 : f0 - 1;  // the warm-up frame: transformed, nothing written
    cf tail[NH];                          // s_{f-1} y'_{f-1}[h + j], j = lane + 64 u
    // ... and s_{f-1} c_{f-1}[h + j] in h words of LDS of the wave's own behind the transform buffers (k_demod_chain_sam)
    cf *ctail = Wn + N + (size_t)W * N + (size_t)wv * h;
#pragma unroll
    for (int u = 0; u < NH; u++) {
        const int j = lane_ + 64 * u;
        tail[u] = make_float2(0.f, 0.f);
        if (j < h) {
            ctail[j] = make_float2(0.f, 0.f);
            if (fs == 0) tail[u] = tl_old[j], ctail[j] = ct_old[j];  // the batch's first frame: the carried tails
        }
    }
    constexpr int NR = (N + 63) / 64;
    constexpr int HO = NR < 3 ? NR : (N <= 512 ? 3 : 2);
    unsigned so[HO];
    idft_slice_offsets<N, HO>(a, cp, lane_, so);
    const int m = cp.m_floor - cp.l, len = cp.r - cp.l;
    cf cC[NH];  // C_f[j], from pass 0 of a frame to its pass 1
#pragma unroll
    for (int u = 0; u < NH; u++) cC[u] = make_float2(0.f, 0.f);
    // ONE loop over (frame, pass): a single copy of the transform in the kernel
    for (int it = 2 * fs; it < 2 * f1; it++) {
        const int f = it >> 1, pass = it & 1;
        const bool emit = f >= f0;
        const float sg = frame_sign(a, cp, f);
        float *out = a.audio + (srow * a.max_batch + f) * h;
        const bool last = (f == F - 1);
        // slice bin t is kept iff lo <= t - m < hi (wave-uniform): the carrier's low-pass, or the sideband
        const int lo = pass == 0 ? -sb.sa.cutoff : (upper ? 0 : -N);
        const int hi = pass == 0 ? sb.sa.cutoff : (upper ? N : 1);
        {
            const int lane = opaque_lane(lane_);
            const Notches nz = notch_load_frame(a, cp.slot);
            cf sv[NR];  // loads first, LDS after
            idft_load_slice_at<N, HO>(a, cp, nz, f, so, lane, sv);
            float pw = 0.f;
#pragma unroll
            for (int u = 0; u < NR; u++) {
                const int t = lane + 64 * u;
                if (t < len) pw += fmaf(sv[u].x, sv[u].x, sv[u].y * sv[u].y);  // (idft_slice_fixed's sum, over the whole window)
                const int d = t - m;
                if (d < lo || d >= hi) sv[u] = make_float2(0.f, 0.f);
            }
            pw = wave_sum(pw);
            idft_slice_fixed<N, R0, R1, R2>(cp, sv, buf, Wn, lane);
            if (pass == 0) {
#pragma unroll
                for (int u = 0; u < NH; u++) {
                    const int j = lane + 64 * u;
                    cC[u] = make_float2(0.f, 0.f);
                    if (j < h) {
                        const cf v0 = buf[j], v1 = buf[h + j];
                        const cf ct = ctail[j];
                        cC[u] = make_float2(__fadd_rn(__fmul_rn(v0.x, sg), ct.x), __fadd_rn(__fmul_rn(v0.y, sg), ct.y));
                        ctail[j] = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                    }
                }
            } else {
                if (emit && lane == 0) a.pwr[srow * a.max_batch + f] = pw;
                int s_nan = 0;
                float lvl = 0.f;
                cf lag = make_float2(0.f, 0.f), ccarry = make_float2(0.f, 0.f);
#pragma unroll
                for (int u = 0; u < NH; u++) {
                    const int j = lane + 64 * u;
                    const cf c = cC[u];
                    cf pr = make_float2(__shfl_up(c.x, 1, 64), __shfl_up(c.y, 1, 64));  // C[j-1]
                    if (lane == 0) pr = ccarry;
                    ccarry = make_float2(__shfl(c.x, 63, 64), __shfl(c.y, 63, 64));
                    if (j < h) {
                        const cf v0 = buf[j], v1 = buf[h + j];
                        const cf y = make_float2(__fmul_rn(v0.x, sg), __fmul_rn(v0.y, sg));
                        const cf ynext = make_float2(__fmul_rn(v1.x, sg), __fmul_rn(v1.y, sg));
                        const cf b = make_float2(__fadd_rn(y.x, tail[u].x), __fadd_rn(y.y, tail[u].y));  // dsp_add_complex :235
                        float mag;
                        const float v = __fmul_rn(2.f, sam_detect(b, c, mag));
                        if (isnan(v)) s_nan = 1;
                        lvl += mag;
                        if (j > 0) {
                            const cf t = sam_lag(c, pr);
                            lag.x += t.x, lag.y += t.y;
                        }
                        if (emit) {
                            out[j] = v;
                            if (last) {  // the two tails of its own move (before the NaN guard); every other mode's state is copied through
                                tl_new[j] = ynext;
                                ct_new[j] = ctail[j];
                                st.bt_new[j] = st.bt_old[j];
                                st.rp_new[j] = st.rp_old[j];
                                if (j == h - 1) a.bb_last[st.row_new] = a.bb_last[st.row_old];
                            }
                        }
                        tail[u] = ynext;
                    }
                }
                const int any_nan = __any(s_nan);
                lvl = wave_sum(lvl);
                lag.x = wave_sum(lag.x), lag.y = wave_sum(lag.y);
                if (emit && lane == 0) {
                    a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
                    sb.sa.car_rec[srow * a.max_batch + f] = make_float2(lvl / (float)h, sb.sa.hz_per_rad * atan2f(lag.y, lag.x));
                }
            }
            wave_lds_sync();  // buf is read out: the next transform may overwrite it
        }
    }
}

// any other n (and n = 360 / 720 with PSDR_DEMOD_CHAIN=0): behind the IDFT kernels on the sideband SAM list (the placed
// ranges), with k_demod_ola_sam's grid.  B' from the client's rows of ypost through ola_step on the client type's own tail;
// the carrier by sam_carrier_dsum over the WHOLE window's kept bins, exactly as k_demod_ola_sam sums it.  The IDFT kernel
// summed pwr over the placed range: the whole window's sum is written here, in idft_slice_fixed's order.
__global__ __launch_bounds__(256) void k_demod_ola_sbsam(DemodArgs a, int nact, SbArgs sb) {
    constexpr int FG = PSDR_OLA_FG;
    const int n = a.n, h = n / 2, tid = threadIdx.x & 63, NT = 64;
    const int F = a.nframes, ngrp = (F + FG - 1) / FG;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nact * ngrp) return;
    const int ci = item / ngrp;
    const ClientParams cp = a.clients[ci];  // [l, r): the placed range
    const SbClient sc = sb.sb[ci];
    ClientParams cw = cp;  // the whole window: the carrier's and pwr's
    cw.l = sc.l, cw.r = sc.r;
    const int f0 = (item - ci * ngrp) * FG;
    const size_t srow = (size_t)cp.slot;
    const cf *yp = a.ypost + (srow * a.max_batch) * n;  // this client's frames
    const SlotState st = slot_state(a, cp, h);
    SlotState sm = st;  // the tail ola_step adds and moves: the client type's own
    sm.bt_old = sb.tail + st.row_old * h, sm.bt_new = sb.tail + st.row_new * h;
    const cf *ct_old = sb.sa.car_tail + st.row_old * h;
    cf *ct_new = sb.sa.car_tail + st.row_new * h;
    const Notches nz = notch_load(a, cp.slot);
    // kept AND placed AND inside the slice (k_demod_ola_sam), of the whole window
    const int m = cw.m_floor - cw.l, len = cw.r - cw.l;
    int d0 = -sb.sa.cutoff, d1 = sb.sa.cutoff;
    if (d0 < -(h - 1)) d0 = -(h - 1);
    if (d0 < -m) d0 = -m;
    if (d1 > h) d1 = h;
    if (d1 > len - m) d1 = len - m;
    for (int g = 0; g < FG; g++) {
        const int f = f0 + g;
        if (f >= F) break;
        const cf *S = a.spec + (size_t)f * a.spec_stride;
        float pw = 0.f;
        for (int t = tid; t < len; t += NT) {
            const cf v = notched(nz, cw, t) ? make_float2(0.f, 0.f) : S[a.lay.pos(cw.l + t)];
            pw += fmaf(v.x, v.x, v.y * v.y);
        }
        pw = wave_sum(pw);
        if (tid == 0) a.pwr[srow * a.max_batch + f] = pw;
        const float sg = frame_sign(a, cw, f), sgp = frame_sign(a, cw, f - 1);
        float *out = a.audio + (srow * a.max_batch + f) * h;
        int s_nan = 0;
        const bool last = (f == F - 1);
        float lvl = 0.f;
        cf lag = make_float2(0.f, 0.f), ccarry = make_float2(0.f, 0.f);
        for (int j0 = 0; j0 < h; j0 += NT) {  // (every lane walks every round: the shuffles below need the whole wave)
            const int j = j0 + tid;
            const bool ok = j < h;
            cf c = make_float2(0.f, 0.f);
            if (ok) {
                const cf cy = sam_carrier_dsum(a, cw, nz, S, d0, d1, j);
                cf ct;
                if (f == 0) {
                    ct = ct_old[j];
                } else {
                    const cf cp1 = sam_carrier_dsum(a, cw, nz, S - a.spec_stride, d0, d1, h + j);
                    ct = make_float2(__fmul_rn(cp1.x, sgp), __fmul_rn(cp1.y, sgp));
                }
                c = make_float2(__fadd_rn(__fmul_rn(cy.x, sg), ct.x), __fadd_rn(__fmul_rn(cy.y, sg), ct.y));
            }
            cf pr = make_float2(__shfl_up(c.x, 1, 64), __shfl_up(c.y, 1, 64));  // C[j-1]
            if (tid == 0) pr = ccarry;
            ccarry = make_float2(__shfl(c.x, 63, 64), __shfl(c.y, 63, 64));
            if (ok) {
                ola_step(a, sm, yp, f, j, [&](cf b) {
                    float mag;
                    const float v = __fmul_rn(2.f, sam_detect(b, c, mag));
                    out[j] = v;
                    if (isnan(v)) s_nan = 1;
                    lvl += mag;
                    if (j > 0) {
                        const cf t = sam_lag(c, pr);
                        lag.x += t.x, lag.y += t.y;
                    }
                    if (last) {  // the carrier's tail moves with the baseband's
                        const cf cn = sam_carrier_dsum(a, cw, nz, S, d0, d1, h + j);
                        ct_new[j] = make_float2(__fmul_rn(cn.x, sg), __fmul_rn(cn.y, sg));
                    }
                });
                if (last) {  // (ola_step moved the client type's own tail as AM's: the AM / FM state is copied through instead)
                    st.bt_new[j] = st.bt_old[j];
                    if (j == h - 1) a.bb_last[st.row_new] = a.bb_last[st.row_old];
                }
            }
        }
        const int any_nan = __any(s_nan);
        lvl = wave_sum(lvl);
        lag.x = wave_sum(lag.x), lag.y = wave_sum(lag.y);
        if (tid == 0) {
            a.nan_flags[srow * a.max_batch + f] = any_nan ? 1 : 0;
            sb.sa.car_rec[srow * a.max_batch + f] = make_float2(lvl / (float)h, sb.sa.hz_per_rad * atan2f(lag.y, lag.x));
        }
    }
}

// ---- auto-notch: the detector behind a batch's last demodulation kernel (include/psdr.h: psdr_client_set_auto_notch) ------
// One wave (one work-group of 64 threads) per auto-notch client of the batch.  It sums the power of the client's UN-notched
// window bins over `period` frames - half a second - in acc[slot][t], then evaluates: the mean over the window, which of the
// slot's two automatic entries stay (some bin above 8 x mean), which local maxima above 16 x mean become new entries
// [l + t - 1, l + t + 2).  It writes the table the demodulation kernels of THIS batch have just read (DemodArgs::notch_auto,
// same stream): a decision made during batch b is in force from batch b + 1.  Lane i owns the bins t = i + 64 k in every loop;
// a bin's sum grows in frame order, the window's sum per lane in ascending t and across lanes through wave_sum's xor tree:
// the bits do not depend on the batch split.  Non-finite sums compare false everywhere: they set nothing and keep nothing.
struct NotchArgs {
    const ClientParams *det;  // [nact] the batch's auto-notch clients: l, r, m_floor, the client's OWN mode, slot
    float *acc;               // [slots][n]
    int *cnt;                 // [slots] frames summed since the last evaluation
    int4 *tab;                // [slots] DemodArgs::notch_auto
    int period;               // max(1, audio_rate / audio_fft_size) frames
};
__global__ __launch_bounds__(64) void k_notch_detect(DemodArgs a, int nact, NotchArgs na) {
    const int lane = threadIdx.x, ci = blockIdx.x;
    if (ci >= nact) return;
    const ClientParams cp = wave_uniform(na.det[ci]);
    const int len = cp.r - cp.l, m = cp.m_floor - cp.l;
    if (len <= 0) return;
    float *acc = na.acc + (size_t)cp.slot * a.n;  // (len <= n: psdr_client_set_audio_range)
    int cnt = na.cnt[cp.slot];
    const int4 e0 = na.tab[cp.slot];
    int ef[2] = {e0.x, e0.z}, ee[2] = {e0.y, e0.w};
    const bool carrier = cp.mode == 2 || cp.mode == 3 || cp.mode == 5;  // AM, FM, SAM: the wanted carrier sits at m
    int f = 0;
    while (f < a.nframes) {
        const int fe = min(a.nframes, f + na.period - cnt);
        for (int t = lane; t < len; t += 64) {
            const cf *S = a.spec + a.lay.pos(cp.l + t);
            float s = acc[t];
            for (int g = f; g < fe; g++) {
                const cf v = S[(size_t)g * a.spec_stride];
                s += fmaf(v.x, v.x, v.y * v.y);
            }
            acc[t] = s;
        }
        cnt += fe - f;
        f = fe;
        if (cnt < na.period) break;
        // evaluate (every lane reads its neighbours' sums: one wave, but through memory)
        __threadfence_block();
        __syncthreads();
        float part = 0.f;
        for (int t = lane; t < len; t += 64) part += acc[t];
        const float mean = wave_sum(part) / (float)len;
        const float keep_thr = 8.f * mean, new_thr = 16.f * mean;
        for (int k = 0; k < 2; k++) {
            if (ee[k] <= ef[k]) continue;
            bool keep = false;
            for (int b = ef[k]; b < ee[k]; b++) {
                const int t = b - cp.l;
                if (t >= 0 && t < len && acc[t] > keep_thr) keep = true;
            }
            if (!keep) ef[k] = ee[k] = 0;
        }
        for (int k = 0; k < 2; k++) {
            if (ee[k] > ef[k]) continue;
            int best = -1;
            float bv = 0.f;
            for (int t = lane; t < len; t += 64) {
                const float x = acc[t], lf = t > 0 ? acc[t - 1] : 0.f, rt = t + 1 < len ? acc[t + 1] : 0.f;
                const int d = t - m;
                const bool prot = carrier && d >= -3 && d <= 3;
                bool ok = !prot && x >= lf && x > rt && x > new_thr;
                const int nf = cp.l + t - 1, ne = cp.l + t + 2;
                for (int q = 0; q < 2; q++)
                    if (ee[q] > ef[q] && nf < ee[q] && ef[q] < ne) ok = false;  // overlaps a set entry
                if (ok && (best < 0 || x > bv)) best = t, bv = x;  // (ascending t: a tie stays with the lower one)
            }
#pragma unroll
            for (int dd = 32; dd > 0; dd >>= 1) {
                const float ov = __shfl_xor(bv, dd, 64);
                const int ot = __shfl_xor(best, dd, 64);
                if (ot >= 0 && (best < 0 || ov > bv || (ov == bv && ot < best))) best = ot, bv = ov;
            }
            if (best >= 0) ef[k] = cp.l + best - 1, ee[k] = cp.l + best + 2;
        }
        __syncthreads();  // every lane has read what it needs of acc
        for (int t = lane; t < len; t += 64) acc[t] = 0.f;
        cnt = 0;
    }
    if (lane == 0) {
        na.cnt[cp.slot] = cnt;
        na.tab[cp.slot] = make_int4(ef[0], ee[0], ef[1], ee[1]);
    }
}

}  // namespace psdr
