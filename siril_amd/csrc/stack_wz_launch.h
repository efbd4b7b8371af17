// stack_wz_launch.h -- host side of the WINSORIZED moment path (kernels:
// stack_wz.h) for columns of 65..1024 samples: the launch is cut into chunks
// of pixels whose records fit the workspace, and each chunk runs three stages
// -- prep (gather, sort, rank record, moments), rounds (the rejection rounds
// on the record) and tails (the pixels the rounds handed to the
// register-resident sorted kernel and to the exact kernel).
//
// Forms (KParams::wz_form, SGPU_WZ):
//   overlapped  float and 16-bit, N <= 128: the workspace is split in two and
//               the prep of chunk k + 1 runs on a second stream while the
//               rounds of chunk k run on the caller's (prep is latency /
//               memory bound, the rounds VALU bound; config 2: 16.13 -> 15.81
//               ms);
//   fused       float, N = 65..128: one kernel does the prep and the capped
//               rounds head; one stream and one workspace buffer per chunk;
//   serial      N > 128 (NP = 512: 52.4 vs 53.2 ms overlapped, twice the
//               chunks of 0.9 M pixels) and SGPU_WZ=4: one stream, one buffer,
//               the tails after the last chunk.
// Float overlapped and fused launches run each chunk's tails on a third
// stream right after its rounds, under the next chunks' prep and rounds.
// Included by stack_sorted_inst.h (KernelFn, FusedFn, the real-slot pickers).
#pragma once

namespace sgpu {

__global__ void k_stack_exact_lds(KParams p, int all_pixels);
__global__ void k_stack_exact_wave(KParams p, int all_pixels);

// total of the chunks' exact-kernel pixels (sgpu_last_exact_pixels)
template <int D>
__global__ void k_add_count(const int *src, int *dst) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(dst, *src * D);
}

// second stream and events of the overlapped form, and the third stream of
// the per-chunk tails, per host thread and device (contexts on different
// threads never share them)
struct WzAux {
    hipStream_t s2 = nullptr, s3 = nullptr;
    hipEvent_t start, prep[2], rounds[2], tails;
};
inline int wz_aux(WzAux *&a) {
    thread_local WzAux tab[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    a = &tab[dev & 15];
    if (!a->s2) {
        if (hipStreamCreateWithFlags(&a->s2, hipStreamNonBlocking) != hipSuccess) return -1;
        if (hipStreamCreateWithFlags(&a->s3, hipStreamNonBlocking) != hipSuccess) return -1;
        hipEvent_t *ev[6] = {&a->start, &a->prep[0], &a->prep[1], &a->rounds[0], &a->rounds[1], &a->tails};
        for (hipEvent_t *e : ev)
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return -1;
    }
    return 0;
}

// LDS scratch threads per block of the exact kernel (sgpu_capi.cpp exact_lds_block)
inline int wz_exact_block(int N) {
    const long long per = 24ll * N;
    int t = 64;
    while (t > 4 && (long long)t * per > 65536) t >>= 1;
    return (long long)t * per <= 65536 ? t : 0;
}

// Where the fused kernel (k_stack_wz_fused1) is the default: the launches on
// which it measured clearly faster than the two-kernel path under the rule of
// DESIGN.md section 8 (every run below every run of the other, medians three
// ranges apart; profiles/r11_ab_wz_fused.txt): unshifted, unnormalized frames
// at sigma 3/3 -- N = 100 8.32 -> 7.80 ms, N = 128 11.59 -> 10.67 ms, one
// rank's 500-row band 1.54 -> 1.44 ms.  Shifted frames (11.01 -> 11.12 ms)
// and sigma 2/2 (30.6 -> 32.8 ms: four pixels in five outlast the head, and
// the tails then run beside nothing) measured slower and keep the two
// kernels, as does every sigma below 3 (not measured; larger sigmas defer
// less than 3/3).  SGPU_WZ=7 fuses wherever the kernel exists.
inline bool wz_fused_auto(const KParams &p) { return !p.shiftx && p.sig0 >= 3.f && p.sig1 >= 3.f; }

// bytes of one of the workspace's nbuf buffers
inline long long wz_buffer_bytes(long long ws_bytes, int nbuf) { return (ws_bytes / nbuf) & ~4095LL; }

// Pixels per chunk (a multiple of 256, or <= 0 when not even one such chunk
// fits): R rank slots per pixel in a workspace of ws_bytes cut into nbuf
// buffers, at most wz_chunk when that is set (SGPU_WZ_CHUNK)
inline long long wz_chunk_pixels(int NP, int R, long long ws_bytes, int nbuf, long long npix, long long wz_chunk) {
    // per pixel: ranks, moments, meta, state of the split rounds and two lists
    const long long per = (long long)R * 4 + 3 * 8 + 16 + (long long)sizeof(WzState) + 8;
    long long ch = std::min<long long>(npix, ((wz_buffer_bytes(ws_bytes, nbuf) - 4096) / per) & ~255LL);
    // RankStore::fetch: umul24(slot, stride) -- stride < 2^24 and the
    // 32-bit product slot * stride < R * ch < 2^32
    ch = std::min<long long>(ch, (1LL << 23) - 256);
    ch = std::min<long long>(ch, (0xffffffffLL / R) & ~255LL);
    // RankStore::store_buf: NP * ch * 4 <= 2^32 (32-bit byte offsets
    // of the record's regions, negative slots down to -NP)
    ch = std::min<long long>(ch, ((1LL << 32) / (4LL * NP) - 256) & ~255LL);
    if (wz_chunk > 0) ch = std::min<long long>(ch, (wz_chunk + 255) & ~255LL);
    return ch;
}

// One workspace buffer carved for a chunk of ch pixels: ranks, moments, meta,
// state, then the two deferral lists of the split rounds (the 4096 bytes
// wz_chunk_pixels holds back cover the alignment of the moments)
struct WzCarve {
    char *ws;
    long long wsb, ch;
    int R;
    int *lists[2];
    void place(KParams &q, int b) {
        char *base = ws + (long long)b * wsb;
        q.wz_ranks = (float *)base;
        q.wz_mom = (double *)(base + (((long long)R * 4 * ch + 255) & ~255LL));
        q.wz_meta = (int *)((char *)q.wz_mom + 3 * 8 * ch);
        q.wz_state = (void *)((char *)q.wz_meta + 16 * ch);
        lists[0] = (int *)((char *)q.wz_state + (long long)sizeof(WzState) * ch);
        lists[1] = lists[0] + ch;
    }
};

// Stage 1, the prep kernel of a launch: PG lanes per pixel.  Float N = 65..128
// is the one-lane prep (k_stack_wz_prep1, its own real-slot bounds and the
// full network: prep1_kernel_128); elsewhere PG is the sorted kernels' G, with
// the real-slot variant where one is compiled (float, 64 slots per lane).
template <int NP, int PG, int W, int U16>
KernelFn wz_prep_kernel(const KParams &p) {
    const int xf = p.shiftx ? 1 : 0;
    if constexpr (NP == 128 && !U16) {
        static_assert(PG == 1, "float N = 65..128: the one-lane prep");
        return prep1_kernel_128(xf, rs_pick_prep1(p.nframes));
    } else {
        constexpr int PE = NP / PG;
        if constexpr (!U16 && PE == 64) {
            const int prs = rs_pick(PE, PG, p.nframes);
            if (prs < PE)
                if (const KernelFn f = rs_kernel<NP>(0, xf, prs)) return f;
        }
        return xf ? &k_stack_wz_prep<NP, PG, 1, W, PE, U16> : &k_stack_wz_prep<NP, PG, 0, W, PE, U16>;
    }
}

// Stage 2, the rounds of chunk q on stream s.  N <= 128: the rank records
// staged in LDS (R = 40 slots: 10 KB per wave); float columns run them split
// (SGPU_WZ_SPLIT, default 2): the head -- k_stack_wz_rounds_lds, or the fused
// kernel when fused_fn is set, which also is the chunk's prep -- runs at most
// `cap` rounds per pixel and hands the rest, a few lanes of nearly every
// wave, to compacted tail passes on this stream -- before the caller records
// rounds[b], so the chunk's fallback tails (third stream) see every append
// and the next prep into the buffer finds records, state and lists free.
// Tail pass 1 defers again, the last one finishes.  N > 128: global reads.
// The tail passes read the head's records: the fused kernel's depth after it
// (fused_kt: wz_fused_kt of the launch's real-slot bucket).
//
// Tail passes (wz_tail_passes): two where the second has work -- at sigma 2/2
// four pixels in five outlast the head and a single pass to the end lost; one,
// run to the end, when both sigmas are >= 3: pass 2 then takes 0.4 % of the
// pixels in 0.06 ms of launch and latency per chunk on the stream everything
// else waits for, and pass 1 finishing them costs less.
// SGPU_WZ_TAIL_PASSES = 1 / 2 (compile time) fixes the count for A/B runs.
inline int wz_tail_passes(const KParams &p) {
    if (SGPU_WZ_TAIL_PASSES) return SGPU_WZ_TAIL_PASSES;
    return p.sig0 >= 3.f && p.sig1 >= 3.f ? 1 : 2;
}
// LDS a fused block asks for at launch: the tiles of its four waves, R = 2 kt
// + KM slots each, at the deeper record; at SGPU_WZ_KT the kernel declares
// them itself (k_stack_wz_fused1)
inline size_t wz_fused_lds_bytes(int kt) {
    return kt == SGPU_WZ_KT ? 0 : (size_t)4 * (2 * kt + SGPU_WZ_KM) * 64 * sizeof(float);
}
template <int NP, int PG, int KTP>
void wz_launch_tail(const KParams &q, const WzSplit &sp, int last, hipStream_t s) {
    // 4 blocks per stripe: 4096 waves at 1024 stripes, the chip's 16 per CU
    hipLaunchKernelGGL((k_stack_wz_tail<NP, PG, KTP>), dim3((unsigned)sp.nstripes * 4u), 64, 0, s, q, sp, last);
}
template <int NP, int PG, int U16>
bool wz_launch_rounds(const KParams &p, const KParams &q, FusedFn fused_fn, int fused_kt, int *const *lists,
                      hipStream_t s) {
    if constexpr (NP > 128) {
        hipLaunchKernelGGL((k_stack_wz_rounds<NP, U16, PG>), (unsigned)((q.wz_cnt + 255) / 256), 256, 0, s, q);
    } else if constexpr (U16) {
        hipLaunchKernelGGL((k_stack_wz_rounds_lds<NP, 1, PG>), dim3((unsigned)((q.wz_cnt + 63) / 64)), 64, 0, s, q,
                           WzSplit{});   // 16-bit: the one nest
    } else {
        const unsigned nblk = (unsigned)((q.wz_cnt + 63) / 64);
        WzSplit sp{};
        if (p.wz_split > 0 && p.wz_scnt) {
            sp.cap = p.wz_split;
            sp.bps = (int)((nblk + kWzStripes - 1) / kWzStripes);
            sp.nstripes = (int)((nblk + sp.bps - 1) / sp.bps);
            sp.list_out = lists[0];
            sp.cnt_out = p.wz_scnt;
            if (hipMemsetAsync(p.wz_scnt, 0, 2 * kWzStripes * kWzStripeStep * sizeof(int), s) != hipSuccess)
                return false;
        }
        if (fused_fn) {
            KParams qa = q;
            WzSplit spa = sp;
            void *args[] = {&qa, &spa};
            if (hipLaunchKernel((const void *)fused_fn, dim3((nblk + 3) / 4), dim3(256), args,
                                wz_fused_lds_bytes(fused_kt), s) != hipSuccess)
                return false;
        } else
            hipLaunchKernelGGL((k_stack_wz_rounds_lds<NP, 0, PG>), dim3(nblk), 64, 0, s, q, sp);
        const int passes = wz_tail_passes(p);
        for (int pass = 0; sp.cap && pass < passes; pass++) {
            sp.list_in = lists[pass & 1];
            sp.cnt_in = p.wz_scnt + (pass & 1) * kWzStripes * kWzStripeStep;
            sp.list_out = lists[(pass + 1) & 1];
            sp.cnt_out = p.wz_scnt + ((pass + 1) & 1) * kWzStripes * kWzStripeStep;
            sp.def = p.wz_def ? p.wz_def + pass : nullptr;
            const int last = pass == passes - 1 ? 1 : 0;
            if (fused_fn && fused_kt != SGPU_WZ_KT) wz_launch_tail<NP, PG, SGPU_WZ_KT_FUSED>(q, sp, last, s);
            else wz_launch_tail<NP, PG, SGPU_WZ_KT>(q, sp, last, s);
        }
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 3, the per-chunk tails of chunk q (float) on the third stream, from
// the chunk-local lists: its fallbacks (the register-resident sorted kernel),
// its deferred pixels (the exact kernel, et threads per block in the LDS
// form) and their count into the launch's total
template <int NP, int G, int RT, int W>
bool wz_launch_tails(const KParams &p, const KParams &q, int et, hipStream_t s3) {
    const unsigned lg = (unsigned)std::min<long long>((q.wz_cnt * G + 255) / 256, 512);
    if (p.shiftx) hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 1, W, 0, 1>), lg, 256, 0, s3, q);
    else hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 0, W, 0, 1>), lg, 256, 0, s3, q);
    // the chunk's deferred pixels: one wave each (stack_exact_wave.hip;
    // SGPU_EXACT_WAVE=0: the one-thread LDS kernel)
    static const bool wave = !std::getenv("SGPU_EXACT_WAVE") || std::atoi(std::getenv("SGPU_EXACT_WAVE")) != 0;
    if (wave) {
        const size_t lds = (size_t)5 * ((p.nframes + 1) & ~1) * sizeof(float);
        const unsigned wb = (unsigned)std::max<long long>(1, std::min<long long>(q.wz_cnt, 1024));
        hipLaunchKernelGGL(k_stack_exact_wave, dim3(wb), dim3(64), lds, s3, q, 0);
    } else {
        const size_t lds = (size_t)et * 24ull * p.nframes;
        const long long per_cu = std::max<long long>(1, (long long)((160ull << 10) / lds));
        const long long eb = std::max<long long>(1, std::min<long long>((q.wz_cnt + et - 1) / et, 256 * per_cu));
        hipLaunchKernelGGL(k_stack_exact_lds, dim3((unsigned)eb), dim3(et), lds, s3, q, 0);
    }
    hipLaunchKernelGGL(k_add_count<1>, dim3(1), dim3(1), 0, s3, (const int *)q.fb_count, p.wz_tcnt + 2 * kWzMaxChunks);
    return hipGetLastError() == hipSuccess;
}

// The launch: 0 done, 1 not on this path (no chunk fits), -1 error
template <int NP, int G, int RT, int W, int U16>
int wz_launch(const KParams &p, hipStream_t s) {
    // the prep's lanes per pixel (the rounds kernels take it as a template argument)
    constexpr int PG = (NP == 128 && !U16) ? 1 : G;
    constexpr int PW = (NP == 128 && !U16) ? SGPU_WZ_PREP_W128_G1 : W;
    const bool fused = NP == 128 && !U16 &&
                       (p.wz_form == kWzFused || (p.wz_form == kWzAuto && wz_fused_auto(p)));
    // slots of the record of the form that runs (chunk size, carving)
    int fused_kt = SGPU_WZ_KT;
    if constexpr (NP == 128 && !U16) fused_kt = wz_fused_kt(rs_pick_prep1(p.nframes));
    const int R = fused ? 2 * fused_kt + RankStore<NP, PG>::KM : RankStore<NP, PG>::R;
    const bool ovl = !fused && p.wz_form != kWzSerial && NP <= 128;
    const int nbuf = ovl ? 2 : 1;
    // the fused form's deeper record may use the whole workspace; the other
    // forms chunk within kWzWsTwoKernel of it, as they were measured
    const long long ws_bytes = fused ? p.wz_ws_bytes : std::min(p.wz_ws_bytes, kWzWsTwoKernel);
    const long long ch = wz_chunk_pixels(NP, R, ws_bytes, nbuf, p.npix, p.wz_chunk);
    if (ch <= 0) return 1;
    WzAux *aux = nullptr;
    hipStream_t sp = s;                      // the prep kernels' stream
    if (fused && wz_aux(aux)) return -1;     // (the third stream and rounds[])
    if (ovl) {
        if (wz_aux(aux)) return -1;
        sp = aux->s2;
        if (hipEventRecord(aux->start, s) != hipSuccess || hipStreamWaitEvent(sp, aux->start, 0) != hipSuccess)
            return -1;
    }
    // per-chunk tails (KParams::wz_tcnt).  (16-bit: the tails run after the
    // last chunk -- the LDS exact kernel of the per-chunk form is the float one)
    const long long nch = (p.npix + ch - 1) / ch;
    const int et = wz_exact_block(p.nframes);
    const bool tails = !U16 && (ovl || fused) && p.wz_tcnt && nch <= kWzMaxChunks && et > 0;
    KernelFn prep_fn = nullptr;
    FusedFn fused_fn = nullptr;
    if constexpr (NP == 128 && !U16) {
        if (fused && !(fused_fn = fused1_kernel_128(p.shiftx ? 1 : 0, rs_pick_prep1(p.nframes)))) return -1;
    }
    if (!fused && !(prep_fn = wz_prep_kernel<NP, PG, PW, U16>(p))) return -1;
    KParams q = p;
    WzCarve cv{(char *)p.wz_ws, wz_buffer_bytes(ws_bytes, nbuf), ch, R, {nullptr, nullptr}};
    int k = 0;
    for (long long p0 = 0; p0 < p.npix; p0 += ch, k++) {
        const int b = k % nbuf;
        cv.place(q, b);
        q.wz_pix0 = p0;
        q.wz_cnt = std::min(ch, p.npix - p0);
        if (tails) {
            q.fb2_list = p.fb2_list + p0;
            q.fb2_count = p.wz_tcnt + 2 * k;
            q.fb_list = p.fb_list + p0;
            q.fb_count = p.wz_tcnt + 2 * k + 1;
        }
        // the buffer's previous chunk must be through its rounds
        if (ovl && k >= nbuf && hipStreamWaitEvent(sp, aux->rounds[b], 0) != hipSuccess) return -1;
        // (fused: no prep launch, the rounds stage launches the fused kernel)
        if (!fused && !launch_fn(prep_fn, (unsigned)((q.wz_cnt * PG + 255) / 256), 256, sp, q)) return -1;
        if (ovl && (hipEventRecord(aux->prep[b], sp) != hipSuccess || hipStreamWaitEvent(s, aux->prep[b], 0) != hipSuccess))
            return -1;
        if (!wz_launch_rounds<NP, PG, U16>(p, q, fused_fn, fused_kt, cv.lists, s)) return -1;
        if ((ovl || (fused && tails)) && hipEventRecord(aux->rounds[b], s) != hipSuccess) return -1;
        if constexpr (!U16) {
            if (tails) {
                if (hipStreamWaitEvent(aux->s3, aux->rounds[b], 0) != hipSuccess) return -1;
                if (!wz_launch_tails<NP, G, RT, W>(p, q, et, aux->s3)) return -1;
            }
        }
    }
    if (tails) {   // the launch ends when every chunk's tails have
        if (hipEventRecord(aux->tails, aux->s3) != hipSuccess || hipStreamWaitEvent(s, aux->tails, 0) != hipSuccess)
            return -1;
        return 0;
    }
    // every prep was joined into s by its rounds: the register-resident
    // kernel over the whole launch's fallbacks runs on s after all of them --
    // enough groups to fill the chip, grid-stride over the list
    const unsigned lgrid = (unsigned)std::min<long long>((p.npix * G + 255) / 256, 2048);
    if (p.shiftx) hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 1, W, U16, 1>), lgrid, 256, 0, s, p);
    else hipLaunchKernelGGL((k_stack_sorted<NP, G, RT, 0, W, U16, 1>), lgrid, 256, 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace sgpu
