// stack_sorted_gw.h -- per column capacity NP, the lane-group width G and
// occupancy target W of the sorted-path kernels ("G, W"): straight rejection
// types (SGPU_GW<NP>) and loop types with data-dependent trip counts
// (SGPU_GW<NP>_LOOP; also the moment path's prep kernel).  Chosen by
// measurement (scripts/exp_variants.sh); -D overrides for variant sweeps.
#pragma once
#ifndef SGPU_GW16
#define SGPU_GW16 1, 4
#endif
#ifndef SGPU_GW16_LOOP
#define SGPU_GW16_LOOP 1, 4
#endif
#ifndef SGPU_GW32
#define SGPU_GW32 1, 4
#endif
#ifndef SGPU_GW32_LOOP
#define SGPU_GW32_LOOP 1, 4
#endif
#ifndef SGPU_GW64
#define SGPU_GW64 1, 3
#endif
#ifndef SGPU_GW64_LOOP
#define SGPU_GW64_LOOP 1, 3
#endif
#ifndef SGPU_GW128
#define SGPU_GW128 1, 2
#endif
#ifndef SGPU_GW128_LOOP
#define SGPU_GW128_LOOP 2, 4
#endif
#ifndef SGPU_GW256
#define SGPU_GW256 2, 2
#endif
#ifndef SGPU_GW256_LOOP
#define SGPU_GW256_LOOP 4, 3
#endif
#ifndef SGPU_GW512
#define SGPU_GW512 4, 3
#endif
#ifndef SGPU_GW512_LOOP
#define SGPU_GW512_LOOP 8, 3
#endif
#ifndef SGPU_GW1024
#define SGPU_GW1024 8, 2
#endif
#ifndef SGPU_GW1024_LOOP
#define SGPU_GW1024_LOOP 16, 3
#endif
// The moment path's float prep kernel at NP = 128 has its own lanes per pixel
// (the rounds kernels take it as a template argument; the fallback sorted
// kernel keeps SGPU_GW128_LOOP's G): 4 (E = 32 slots per lane), 2 (E = 64) or
// 1 (the whole column in one lane: k_stack_wz_prep1, stack_wz.h), for
// unshifted frames and for shifted / normalized ones (XF) separately.
// Its occupancy target -- waves per SIMD the register allocation must allow
// -- per form: SGPU_WZ_PREP_W128 for four lanes, _G2 for two, _G1 for one.
#ifndef SGPU_WZ_PREP_G128
#define SGPU_WZ_PREP_G128 1
#endif
#ifndef SGPU_WZ_PREP_G128_XF
#define SGPU_WZ_PREP_G128_XF 1
#endif
#ifndef SGPU_WZ_PREP_W128
#define SGPU_WZ_PREP_W128 6
#endif
#ifndef SGPU_WZ_PREP_W128_G2
#define SGPU_WZ_PREP_W128_G2 4
#endif
// (one lane: 159-162 VGPRs, three waves per SIMD, with either 2 or 3 here)
#ifndef SGPU_WZ_PREP_W128_G1
#define SGPU_WZ_PREP_W128_G1 3
#endif
// the fused prep + rounds kernel (k_stack_wz_fused1): the one-lane prep's budget
#ifndef SGPU_WZ_FUSED_W128
#define SGPU_WZ_FUSED_W128 3
#endif
// real-slot bounds of the four-lane prep (stack_sorted_rs128.hip): first
// bound and step; rs_pick_prep4 takes the smallest one >= ceil(N / 4)
#ifndef SGPU_WZ_PREP4_RS0
#define SGPU_WZ_PREP4_RS0 20
#endif
#ifndef SGPU_WZ_PREP4_RSSTEP
#define SGPU_WZ_PREP4_RSSTEP 4
#endif
static_assert((SGPU_WZ_PREP_G128 == 1 || SGPU_WZ_PREP_G128 == 2 || SGPU_WZ_PREP_G128 == 4) &&
              (SGPU_WZ_PREP_G128_XF == 1 || SGPU_WZ_PREP_G128_XF == 2 || SGPU_WZ_PREP_G128_XF == 4),
              "prep kernel: 1, 2 or 4 lanes per pixel");
