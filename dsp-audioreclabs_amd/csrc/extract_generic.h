// extract_generic.h -- the extraction clip body for the runtime LDS layout (ExtractParams::cv),
// and the helpers that only it uses.  Part of extract.hip, which includes it after the types and
// the helpers it shares with the compile-time (FAST) layout's clip_fast.
//
// clip_body<EXACT> serves clips of any length the launch's layout holds: clips longer than the
// register file are read word by word, more than 128 / 256 VAD or feature frames take the ballot
// and rank paths.  Two callers: extract_kernel<false> (EXACT = false: launches that do not fit the
// FAST layout) and extract_exact_kernel (EXACT = true: the near-tie redo of every launch).
#ifndef DSP_EXTRACT_GENERIC_H
#define DSP_EXTRACT_GENERIC_H

namespace dsp {

// one buffer word (four 16-B vectors) of a clip longer than the register file, from L2
__device__ __forceinline__ void issue_word(short8 *q, const ExtractParams &p, const ClipRef &c, int w)
{
    const __amdgpu_buffer_rsrc_t rs = clip_rsrc(p, c);
#pragma unroll
    for (int k = 0; k < 4; k++)
        q[k] = __builtin_bit_cast(short8, __builtin_amdgcn_raw_buffer_load_b128(rs, 64 * w + 16 * k, 0, 0));
}

// R1 of one 32-sample buffer word w of a clip (lead, n, nword): exact moments (sum k, sum k^2) to
// wS1[w] / wS2[w]; the thread's running sum K, min and max in a (packed int16 min / max for the
// interior words, whose 32 samples are all the clip's)
__device__ __forceinline__ void r1_word(const short8 *q, int w, int nword, int lead, int n, R1Acc &a, int *wS1,
                                        unsigned long long *wS2)
{
    int s1 = 0;
    unsigned long long s2 = 0;
    if (w > 0 && w < nword - 1) {  // all 32 samples are the clip's
        const short2v ones = {1, 1};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const short2v d = half_pair(q[k], h);
                a.pmin = __builtin_elementwise_min(a.pmin, d);
                a.pmax = __builtin_elementwise_max(a.pmax, d);
                s1 = __builtin_amdgcn_sdot2(d, ones, s1, false);
                s2 += (unsigned)sq2(d);  // <= 2^31: unsigned
            }
    } else {  // first / last word of the clip: real samples only
        // select among values (v_cndmask), never among pointers into the caller's register array:
        // a pointer select in a rolled loop moves the whole array to scratch
        const short8 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const short8 v = k == 0 ? q0 : k == 1 ? q1 : k == 2 ? q2 : q3;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int u = 32 * w + 8 * k + e;
                const int x = v[e];
                if (u >= lead && u < lead + n) {
                    s1 += x;
                    s2 += (unsigned)(x * x);
                    a.kmin = min(a.kmin, x);
                    a.kmax = max(a.kmax, x);
                }
            }
        }
    }
    wS1[w] = s1;
    wS2[w] = s2;
    a.K += s1;
}

// the wave's R1 partials -> sh->red_*[wid] (every lane of the wave active)
__device__ __forceinline__ void r1_reduce(const R1Acc &a, Shared *sh, int wid, int lane)
{
    const int kmn = min(a.kmin, min((int)a.pmin.x, (int)a.pmin.y));
    const int kmx = max(a.kmax, max((int)a.pmax.x, (int)a.pmax.y));
    const long long ks = (long long)wave_sum(a.K);  // <= 64 threads' sums < 2^31
    const int wmn = wave_min(kmn), wmx = wave_max(kmx);
    if (lane == 0) {
        sh->red_k[wid] = ks;
        sh->red_a[wid] = wmn;
        sh->red_b[wid] = wmx;
    }
}

// the clip statistics (ClipStats, extract.hip) from the per-wave partial sums in sh->red_*
__device__ __forceinline__ ClipStats clip_stats(const Shared *sh, int n, int L, int S, int do_vad)
{
    long long Kt = 0;
    int kmin = 0x7fffffff, kmax = -0x7fffffff - 1;
#pragma unroll
    for (int w = 0; w < NWAVE; w++) {
        Kt += sh->red_k[w];
        kmin = min(kmin, sh->red_a[w]);
        kmax = max(kmax, sh->red_b[w]);
    }
    ClipStats s;
    s.mq = uni((double)Kt / (double)n);
    s.Mp = uni(fmax((double)kmax - s.mq, s.mq - (double)kmin));
    s.tpos = uni((int)floor(s.mq) + 1);
    s.t0 = uni((int)floor(s.mq + 0.5));
    s.invMf = uni(s.Mp > 0.0 ? (float)(1.0 / s.Mp) : 0.0f);  // as dsp_extract_general (same bits)
    s.invM2 = uni(s.Mp > 0.0 ? 1.0 / (s.Mp * s.Mp) : 0.0);   // endpoint energies (one rounding)
    s.nv = (do_vad && n >= L) ? (n - L) / S + 1 : 0;
    s.kneg = kmin == -32768;
    return s;
}

// exact moments (sum k, sum k^2) of elements [e0, e1) of one 32-sample word, branch-free: the
// range as a bit mask M; pair p's two bits become a 16-bit-lane mask (v_bfe_i32 of each bit,
// merged by v_bfi), and the pair's masked samples go through one v_dot2 each for sum k and sum k^2
// (a rolled loop with a branch per element cost ~1.9k instructions per clip, a third of them scalar)
__device__ __forceinline__ void partial_moments(const short8 (&q)[4], int e0, int e1, int &t1, unsigned long long &t2)
{
    const uint32_t hi = e1 >= 32 ? ~0u : (1u << e1) - 1u;
    const uint32_t M = hi & ~((1u << e0) - 1u);  // e0 < 32
    const short2v ones = {1, 1};
    int s1 = 0;
    unsigned long long s2 = 0;
    const short8 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];  // value selects (see r1_word)
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const short8 v = k == 0 ? q0 : k == 1 ? q1 : k == 2 ? q2 : q3;
        const uint32_t Mk = M >> (8 * k);
#pragma unroll
        for (int h = 0; h < 4; h++) {  // pair 4k + h: elements 8k + 2h, 8k + 2h + 1
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_sbfe((int)Mk, 2 * h, 1);
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_sbfe((int)Mk, 2 * h + 1, 1);
            const uint32_t m = (b0 & 0x0000FFFFu) | (b1 & 0xFFFF0000u);
            const short2v dm = __builtin_bit_cast(short2v, __builtin_bit_cast(uint32_t, half_pair(v, h)) & m);
            s1 = __builtin_amdgcn_sdot2(dm, ones, s1, false);
            s2 += (unsigned)sq2(dm);
        }
    }
    t1 += s1;
    t2 += s2;
}

// Ranks (ties broken by index) of nseq sequences of n elements, element (q, i) = get(q, i).  Wave w
// compares every element with its chunk of the other elements; the partial counts are combined
// with integer LDS atomics (exact, order-free).  rk[nseq * n] must be zeroed before the barrier
// that precedes this call; the ranks are complete after the next barrier.
template <typename Get>
__device__ __forceinline__ void rank_partial(Get get, int nseq, int n, int *rk, int wid, int lane)
{
    const int per = (n + NWAVE - 1) / NWAVE;
    const int jlo = wid * per, jhi = min(n, jlo + per);
    if (jlo >= jhi) return;
    for (int q = 0; q < nseq; q++)
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const auto e = get(q, i < n ? i : 0);
            int r = 0;
#pragma unroll 4
            for (int j = jlo; j < jhi; j++) {
                const auto o = get(q, j);
                r += (o < e) || (o == e && j < i);
            }
            if (i < n && r) atomicAdd(&rk[q * n + i], r);
        }
}


// Order statistics r0 / r1 (ranks with ties broken by index) of v[0..n), n <= 256: every wave
// holds the whole sequence in registers (lane + 64k), wave w ranks elements w, w + NWAVE, ...
// with one ballot per chunk.  Lane 0 of the wave that finds them stores them.
template <typename T, typename Get>
__device__ __forceinline__ void ballot_select(Get get, int n, int r0, int r1, double *o0, double *o1,
                                              int wid, int lane)
{
    T x[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        x[k] = j < n ? get(j) : (T)0;
    }
    const int kc = (n + 63) >> 6;
    for (int i = wid; i < n; i += NWAVE) {
        const int ki = i >> 6;
        const T e = lane_read(ki == 0 ? x[0] : ki == 1 ? x[1] : ki == 2 ? x[2] : x[3], i & 63);
        int r = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < kc) {
                const int j = lane + 64 * k;
                r += __popcll(__ballot(j < n && (x[k] < e || (x[k] == e && j < i))));
            }
        }
        if (lane == 0) {
            if (r == r0) *o0 = (double)e;
            if (r == r1) *o1 = (double)e;
        }
    }
}

// One clip, start to finish; its first RREG words are already in flight into regs (word
// r * NT + tid in regs[4r .. 4r+3]).  EXACT = false: endpoint energies from exact moments,
// decisions certified; returns false on a near tie (the clip is then redone with EXACT = true
// after the persistent loop).
// Runtime LDS layout (p.cv) only: extract_kernel<false>'s clips (EXACT = false) and the exact redo
// of both launch kinds (EXACT = true).  The compile-time layout's clips run clip_fast.
struct NoClaim {
    __device__ int operator()() const { return -1; }
};
template <bool EXACT, typename Resolve = NoClaim>
__device__ __forceinline__ bool clip_body(const ExtractParams &p, const Ctx &c, int i, const ClipRef &cur,
                                          short8 (&regs)[NRV], Resolve resolve = NoClaim())
{
    Shared *sh = c.sh;
    // (this layout's index arithmetic spills when hoisted: opaque thread index)
    const int tid = opaque_tid(), lane = tid & 63,
              wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar branches
    // frame sizes opaque per clip as well: constants derived from them ((double)L, ...) are
    // recomputed in the clip instead of being kept live across the loop
    int L = p.L, S = p.S;
    asm volatile("" : "+s"(L), "+s"(S));
    const int n = cur.n, lead = cur.lead, nword = cur.nword;
    // outputs: the main kernel stages them in LDS (slot i mod EXTRACT_OSTAGE) and the workgroup
    // writes a chunk's clips together (flush_outputs); the exact redo writes them directly
    const int oslot = i & (EXTRACT_OSTAGE - 1);
    float *featb = EXACT ? out_feat(p, i) : reinterpret_cast<float *>(c.orow + DSP_OUT_ROW_WORDS * oslot);
    const int16_t *clip_g = p.pcm + cur.base + lead;  // the clip in global memory, sample coords
    STAMP(i, 0);
    stamp_loads_landed(p, i, wid, lane);

    // ---- R1: integer sum / min / max; exact moments per 32-sample word -----------------------
    R1Acc acc = r1_acc_init();  // K <= RREG * 32 * 32768 per thread (longer clips: one word per trip)
    // clips of up to RREG * NT words stream from the registers loaded before this call; longer
    // ones are read word by word here and again in R2 (the second read hits L2)
    const bool inreg = nword <= RREG * NT;
    if (inreg) {
#pragma unroll
        for (int r = 0; r < RREG; r++) {
            const int w = r * NT + tid;
            if (w < nword) r1_word(&regs[4 * r], w, nword, lead, n, acc, c.wS1, c.wS2);
        }
    } else {
#pragma unroll 1
        for (int w = tid; w < nword; w += NT) {
            short8 q[4];
            issue_word(q, p, cur, w);
            r1_word(q, w, nword, lead, n, acc, c.wS1, c.wS2);
        }
    }
    r1_reduce(acc, sh, wid, lane);
    __syncthreads();
    if constexpr (!EXACT) reset_staged(sh, tid);
    if (wid == 0) share_clip_stats(sh, clip_stats(sh, n, L, S, p.do_vad), lane);
    __syncthreads();
    const ClipStats cs = shared_clip_stats(sh);
    const double mq = cs.mq, Mp = cs.Mp;
    const int tpos = cs.tpos, t0 = cs.t0, nv = cs.nv;
    STAMP(i, 1);

    // ---- R2: positive-sample bits, one 32-bit word per 32 buffer samples ---------------------
    if (inreg) {
#pragma unroll
        for (int r = 0; r < RREG; r++) {
            const int w = r * NT + tid;
            if (w < nword) c.posw[w] = (DSP_ABL & 4) ? 0u : pos_word(&regs[4 * r], w, nword, lead, n, tpos);
        }
    } else {
#pragma unroll 1
        for (int w = tid; w < nword; w += NT) {
            short8 q[4];
            issue_word(q, p, cur, w);
            c.posw[w] = pos_word(q, w, nword, lead, n, tpos);
        }
    }
    if (tid < 2) c.posw[nword + tid] = 0;
    __syncthreads();
    STAMP(i, 2);

    // ---- R3: endpoint detection (:161-273) ------------------------------------------------
    int st = 0, en = n;
    if (nv > 0) {
        // frame f = buffer samples [u0, u0 + L): exact moments from the word sums plus the two
        // partial words at its ends, sign changes from the bits.
        if constexpr (!EXACT) {
            // Pass A, one thread per frame end: the partial word's moments, re-read from L2
            for (int t = tid; t < 2 * nv; t += NT) {
                int e0, e1, t1 = 0;
                unsigned long long t2 = 0;
                const int pw = vad_partial_word(cur, L, S, nv, t, e0, e1);
                if (pw >= 0) {
                    short8 q[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) q[k] = load_vec(p, cur, 4 * pw + k);
                    partial_moments(q, e0, e1, t1, t2);
                }
                c.pS1[t] = t1;
                c.pS2[t] = t2;
            }
            __syncthreads();
            STAMP(i, 7);
        }
        // Pass B, one quad per frame: interior word sums and sign changes, each lane a contiguous
        // quarter
        const int q4 = tid >> 2, lq = tid & 3;
        for (int f0 = 0; f0 < nv; f0 += NT / 4) {
            const int f = f0 + q4;
            const bool act = f < nv;
            int s1 = 0;  // |frame sum| <= L * 32768 < 2^31 for L < 65536
            unsigned long long s2 = 0;
            int zc = 0;
            if (act) {
                const int u0 = lead + f * S, u1 = u0 + L;
                if (!EXACT) {
                    const int wa = u0 >> 5, wb = (u1 - 1) >> 5;
                    const int wi0 = (u0 & 31) ? wa + 1 : wa, wi1 = (u1 & 31) ? wb - 1 : wb;
                    const int per = (wi1 - wi0 + 4) >> 2;
                    const int ws = wi0 + lq * per, we = min(ws + per - 1, wi1);
#pragma unroll 3
                    for (int w = ws; w <= we; w++) {
                        s1 += c.wS1[w];
                        s2 += c.wS2[w];
                    }
                    if (lq == 0) {
                        s1 += c.pS1[2 * f] + c.pS1[2 * f + 1];
                        s2 += c.pS2[2 * f] + c.pS2[2 * f + 1];
                    }
                }
                const int np_ = L - 1, pq = (np_ + 3) >> 2;  // pairs [u0, u1 - 1) in quarters
                const int x0 = u0 + min(lq * pq, np_), x1 = u0 + min((lq + 1) * pq, np_);
                zc = chg_run(c.posw, x0, x1);
            }
            s1 = dpp_quad_reduce(s1, OpAdd());
            s2 = dpp_quad_sum64(s2);
            zc = dpp_quad_reduce(zc, OpAdd());
            if (act && lq == 0) {
                c.rank[f] = 0;
                c.vE[f] = EXACT ? np_energy_exact(clip_g, f * S, L, mq, Mp)
                                : energy_from_moments(s2, s1, L, t0, mq - (double)t0, cs.invM2);
                c.vZ[f] = zc;
            }
        }
        __syncthreads();
        STAMP(i, 8);
        // p90 order statistics (:198)
        const P90Rank<int> pr = p90_rank(nv);
        if (nv <= 128) {
            if (wid == 0) {
                // the workgroup's critical path (p90, then the scan) runs on this one wave: it
                // takes issue priority over the co-resident workgroup's waves until the decisions
                // are made (2% at 100k clips)
                __builtin_amdgcn_s_setprio(2);
                p90_select_wave(c, nv, lane);
            }
        } else if (nv <= 256) {
            ballot_select<double>([&](int j) { return c.vE[j]; }, nv, pr.r0, pr.r1, &sh->pa, &sh->pb, wid, lane);
        } else {  // long clips: partial ranks over all waves
            rank_partial([&](int, int j) { return c.vE[j]; }, 1, nv, c.rank, wid, lane);
            __syncthreads();
            for (int f = tid; f < nv; f += NT) {
                const int r = c.rank[f];
                if (r == pr.r0) sh->pa = c.vE[f];
                if (r == pr.r1) sh->pb = c.vE[f];
            }
        }
        if (wid == 1 % NWAVE) vad_noise(c, nv, lane);  // beside wave 0's p90 selection
        __syncthreads();
        STAMP(i, 3);
        if (wid == 0) {
            const int flag = vad_scan<!EXACT, false>(p, c, nv, lane);
            if (lane == 0) sh->exact = (!EXACT && Mp > 0.0) ? flag : 0;
            __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
        if (!EXACT && sh->exact) return false;  // near tie: redone in numpy's exact order by the exact kernel
        crop_from_scan(sh, L, S, n, st, en);
        dump_vad(p, c, i, nv);
    }
    STAMP(i, 4);

    // ---- R4: windowed frames over the crop [st, en) (r4_frames) --------------------------------
    const int F = r4_frames<false>(p, c, cur, L, S, st, en, cs, sh->j0, sh->j1, wid, lane);
    STAMP(i, 12);
    if (F > 128)  // the long-sequence R5's rank scratch
        for (int t = tid; t < 3 * F; t += NT) c.rank[t] = 0;
    if constexpr (!EXACT)
        if (tid == 0) sh->next = resolve();  // claimed at the clip's start (-1: none)
    __syncthreads();
    if constexpr (!EXACT) {
        // regs are dead since R2: the next clip's words load while R5 runs (unconditional, a
        // clip_none() reads zeros, so the compiler's vmcnt bookkeeping stays exact)
        const int nx = sh->next;
        issue_clip(regs, p, nx >= 0 ? clip_ref(p, nx) : clip_none(), tid);
    }
    STAMP(i, 5);

    // ---- R5: 15-d statistics (compute_statistics x 3, fe.py:46-62) ------------------------
    // np.median: the middle order statistic (odd F) or the mean of the two middle ones
    const int r0 = (F - 1) / 2, r1 = F / 2;
    if (F <= 128) {
        r5_fast(c, F, featb, wid, lane);
    } else {
        // long sequences: partial ranks over all waves (c.rank zeroed above), then one wave per
        // sequence.  (Tried as a function r5_long beside r5_fast: extract_kernel<false> then
        // allocated its registers anew, 2 649 of its 11 815 disassembly lines changed and its
        // figures in tools/kinfo.sh moved; inline, its code stays as it was.)
        rank_partial([&](int q, int j) { return q == 2 ? (float)c.fZ[j] : (q == 0 ? c.fE[j] : c.fM[j]); }, 3, F, c.rank,
                     wid, lane);
        __syncthreads();
        for (int t = tid; t < 3 * F; t += NT) {
            const int q = t / F, e = t - q * F;
            const int r = c.rank[t];
            const double val = q == 2 ? (double)c.fZ[e] : (double)(q == 0 ? c.fE[e] : c.fM[e]);
            if (r == r0) sh->oslo[q] = val;
            if (r == r1) sh->oshi[q] = val;
        }
        __syncthreads();
        if (wid < 3) {
            double s = 0.0, mx = -INFINITY, mn = INFINITY;
            for (int q = lane; q < F; q += 64) {
                const double x = wid == 0 ? (double)c.fE[q] : wid == 1 ? (double)c.fM[q] : (double)c.fZ[q];
                s += x;
                mx = fmax(mx, x);
                mn = fmin(mn, x);
            }
            s = wave_sum(s);
            mx = wave_maxd(mx);
            mn = wave_mind(mn);
            const double mean = s / (double)F;
            double qq = 0.0;
            for (int q = lane; q < F; q += 64) {
                const double x = wid == 0 ? (double)c.fE[q] : wid == 1 ? (double)c.fM[q] : (double)c.fZ[q];
                const double d = x - mean;
                qq = fma(d, d, qq);
            }
            qq = wave_sum(qq);
            double med;
            {
#pragma clang fp contract(off)
                med = (F & 1) ? sh->oshi[wid] : (sh->oslo[wid] + sh->oshi[wid]) / 2.0;
            }
            if (lane < 5) {
                const double o = lane == 0 ? mean : lane == 1 ? sqrt(qq / (double)F) : lane == 2 ? mx : lane == 3 ? mn : med;
                featb[5 * wid + lane] = (float)o;
            }
        }
    }
    STAMP(i, 9);
    if (p.seq)
        for (int g = tid; g < F && g < p.ld_seq; g += NT) {
            float *o = p.seq + ((size_t)i * p.ld_seq + g) * 3;
            o[0] = c.fE[g];
            o[1] = c.fM[g];
            o[2] = (float)c.fZ[g];
        }
    if (tid == 0) {
        if constexpr (EXACT) {
            out_se(p, i)[0] = st;
            out_se(p, i)[1] = en;
            *out_nf(p, i) = F;
            *out_st(p, i) = DSP_CLIP_OK | DSP_CLIP_FLAG_VAD_EXACT;
        } else {
            stage_outputs(c, i, st, en, F);
        }
    }
    STAMP(i, 6);
    return true;
}

}  // namespace dsp
#endif
