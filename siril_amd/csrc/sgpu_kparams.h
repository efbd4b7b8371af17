// sgpu_kparams.h -- kernel parameter block shared by the host C-ABI layer
// (sgpu_capi.cpp) and the HIP kernels.  Plain data, device pointers only.
#pragma once
#include <stdint.h>

namespace sgpu {

// rejection enum, reference core/settings.h:43-52
enum Rejection : int {
    NO_REJEC = 0, PERCENTILE = 1, SIGMA = 2, MAD = 3, SIGMEDIAN = 4,
    WINSORIZED = 5, LINEARFIT = 6, GESDT = 7,
    KMEDIAN = 16   // pseudo type: stack_median (median_and_mean.c:1711-1715)
};
// normalization enum, reference core/settings.h:34-40
enum Normalization : int {
    NO_NORM = 0, ADDITIVE = 1, MULTIPLICATIVE = 2, ADDITIVE_SCALING = 3,
    MULTIPLICATIVE_SCALING = 4
};

// Forms of the WINSORIZED moment path (stack_wz_launch.h), from SGPU_WZ
enum WzForm : int {
    kWzAuto = 0,        // unset: fused where it measured faster (wz_fused_auto), two kernels elsewhere
    kWzTwoKernel,       // 2 (and any other value): prep and rounds kernels everywhere
    kWzFused,           // 7: prep and capped rounds head in one kernel wherever it exists (float, N = 65..128)
    kWzSerial,          // 4: two kernels on one stream, tails after the last chunk (per-kernel times of a profile)
    kWzSortedOnly       // 0: no moment path, the register-resident sorted kernel
};

struct KParams {
    const float *frames;        // frame-major block: frames[f*frame_stride + y*W + x]
    long long frame_stride;     // elements between frames
    long long npix;             // rows * W output pixels
    int W;                      // row length
    int nframes;                // N (nb_images_to_stack)
    int rtype;                  // Rejection (or KMEDIAN)
    float sig0, sig1;           // args->sig[0..1]
    int norm;                   // Normalization
    const double *scale, *offset, *mul;   // per-frame coefficients (device) or null
    const int *shiftx;          // per-frame integer x shift (device) or null
    const double *weights;      // per-frame weights (device) or null
    const float *drizz;         // per-sample drizzle weights, layout of frames (args->drizzle), or null
    const float *mask;          // per-sample feather-mask weights, layout of frames (masking), or null
    const float *crit;          // GESD critical values (device) or null
    float m_x, m_dx2;           // LINEARFIT constants (median_and_mean.c:1487-1500)
    int output_norm;            // 0 -> clamp result to [0,1]
    float *out;                 // rows*W
    uint16_t *rej_lo, *rej_hi;  // rows*W each, or null
    unsigned long long *counts; // [2] low/high rejection totals (accumulated)
    unsigned long long *cstripe;  // striped per-wave partial totals (kCountStripes x 8, reduced into counts) or null
    int *fb_list;               // pixels deferred to the exact sequential kernel
    int *fb_count;              // number of entries in fb_list
    int *fb2_list;              // WINSORIZED moment path: pixels for the register-resident sorted kernel
    int *fb2_count;             // number of entries in fb2_list
    // WINSORIZED moment path (stack_wz.h): pixels [wz_pix0,
    // wz_pix0 + wz_cnt) of this launch, their rank records (slot-major,
    // stride wz_cnt), window moments [2][wz_cnt] and packed bounds / routes
    long long wz_pix0, wz_cnt;
    float *wz_ranks;
    double *wz_mom;
    int *wz_meta;
    void *wz_state;             // split rounds: WzState per pixel of the chunk, written by the head for the pixels
                                // it defers and carried from tail pass to tail pass
    void *wz_ws;                // workspace the launcher carves these from (stack_wz_launch.h), or null
    long long wz_ws_bytes;
    long long wz_chunk;         // at most this many pixels per chunk (0: as the workspace allows)
    int *wz_tcnt;               // overlapped and fused forms: 2 counters per chunk (fb2, fb) + [kWzMaxChunks*2] the total
                                // of the chunks' exact-kernel pixels, or null (tails after the last chunk)
    WzForm wz_form;             // which kernels and streams a WINSORIZED launch of 65..1024 samples takes
    int wz_split;               // LDS rounds, float, N <= 128: rounds cap of the head pass (SGPU_WZ_SPLIT; 0: one nest)
    int *wz_scnt;               // split: stripe counters of the two deferral lists [2][kWzStripes * 16], or null
    int *wz_def;                // split: [2] pixels that entered tail pass 1 / 2 (sgpu_last_wz_deferred), or null
    float *scratch;             // fallback kernel scratch
    long long scratch_threads;  // number of fallback threads the scratch covers
    // DATA_USHORT sequences (apply_rejection_ushort path)
    const uint16_t *frames16;   // non-null: 16-bit input (frames ignored)
    uint16_t *out16;            // 16-bit output (round_to_WORD), or null
    int out_f32;                // 16-bit input: write the float output (double_ushort_to_float_range)
    double out16_mul;           // 16-bit output: result x this before round_to_WORD (normalize_to16bit:
                                // 65535/255 for BYTE_IMG input with output_norm, else 1)
    unsigned long long *prof;   // diagnostic builds (-DSGPU_PROF=1): per-section lane-cycles [16], or null
};

// Split rounds (stack_wz.h, k_stack_wz_rounds_lds / k_stack_wz_tail): the
// pixels a pass hands on go to a striped list.  Stripe s takes the appends of
// the head's blocks [s * bps, (s + 1) * bps) and owns entries [s * bps * 64,
// (s + 1) * bps * 64) of the list -- room for every pixel of those blocks --
// so a wave's append is one atomic on its stripe's counter (counters 64 B
// apart), not on one word for the whole chunk.  A tail pass reads stripe s of
// list_in and appends what it hands on again to stripe s of list_out.  An
// entry names the pixel and the compact copy of its ranks (stack_wz.h,
// wz_entry).
struct WzSplit {
    int cap;                    // rounds per pass (0: head only, no deferral)
    int nstripes, bps;          // stripes in use, head blocks per stripe
    const int *list_in, *cnt_in;
    int *list_out, *cnt_out;
    int *def;                   // tail: the pass's word of KParams::wz_def, or null
};
// Workspace (sgpu_capi.cpp allocates it): the two-kernel forms use at most 2
// GiB of it, the size their chunking was tuned at.  The fused form's record
// (R = 48 slots, 280 bytes a pixel with moments, meta, state and lists) needs
// 2.35 GB for the largest chunk the 23-bit stride allows (8 388 352 pixels):
// at 2 GiB a 24 M-pixel launch would take four chunks where it took three.
// Only a launch that can run the deeper record gets the larger cap: float, at
// least kWzDeepMinFrames frames (real-slot bucket 96 up), fused or auto form.
constexpr long long kWzWsTwoKernel = 2LL << 30;
constexpr long long kWzWsMax = 5LL << 29;   // 2.5 GiB
constexpr int kWzDeepMinFrames = 89;

constexpr int kWzStripes = 1024;
constexpr int kWzStripeStep = 16;   // ints between two stripe counters

// most chunks of one launch whose tails run per chunk (KParams::wz_tcnt)
constexpr int kWzMaxChunks = 256;
// the context's counter block (ints): [0, 2 * kWzMaxChunks] KParams::wz_tcnt,
// then the two words of KParams::wz_def (all zeroed per launch), and from
// kWzScntOff the stripe counters KParams::wz_scnt (zeroed per chunk)
constexpr int kWzDefOff = 2 * kWzMaxChunks + 1;
constexpr int kWzScntOff = 1024;
constexpr int kWzCntInts = kWzScntOff + 2 * kWzStripes * kWzStripeStep;
static_assert(kWzDefOff + 2 <= kWzScntOff, "counter block layout");
// rejection totals: one wave per pixel group ends with one pair of atomics;
// on one address those serialise across the XCDs (hundreds of thousands of
// waves per launch), so waves add into kCountStripes pairs 64 B apart and a
// one-block kernel folds them into `counts` at the end of the launch
constexpr int kCountStripes = 1024;

}  // namespace sgpu
