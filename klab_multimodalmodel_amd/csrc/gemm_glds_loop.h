// The LDS-DMA ring's main loop -- the ONE copy.  NOT a stand-alone header: a fragment #included (three times) inside the bodies
// of csrc/gemm.hip: gemm_glds_body, gemm_glds_w8_body and gemm_glds_fp8_body.  Textual on purpose: as a function of its own the
// loop is optimised before it is inlined and hipcc then schedules and allocates the kernels differently (the 128 x 64 and
// 64 x 64 tiles went from 128 / 76 to 206 / 114 VGPRs); included, every kernel's code is what it was with three literal copies.
//
// Software-pipelined, hand-scheduled.  Per k-tile t a wave: waits until k-tile t+1 has landed (counted vmcnt) + one s_barrier,
// then issues its MFMAs on the fragments of t (already in registers) with the LDS reads of t+1 (other register set) and the
// LDS-DMA of t+S-1 slotted into the gaps between them.  Before this rewrite the three phases ran back to back in each wave
// (measured additive: DMA issue + LDS latency + MFMA).
//
// It owns everything from the zeroed accumulators to the last retired MFMA and LDS-DMA: k-tile rotation, prologue fill, first
// fragment reads, steady loop, tail(s), closing nops and vmcnt(0).
//   in scope before it : OA, OB (GldsOperand types: L, BYTES, NF, RPF, issue1, read1<R, SOFF>) and oa, ob after init();
//                        BM, BN, MI, NI; smem, wave; bm0, bn0, kt0, nt (KLAB_GLDS_WORK)
//   policy, #defined by the including body and #undef-ed here:
//     KLAB_RING_MMA(ACC, A, B)  the MFMA step on one A and one B fragment (bf16 swapped / not swapped for ATOMIC / fp8 pair)
//     KLAB_RING_TWO_BASES       0: one LDS base register + SN * STAGE immediates; 1: two bases + (SN & 1) * STAGE
//     KLAB_RING_DRAIN4          1: compile the pipelined drain of "exactly four k-tiles left" in front of the general tail
//   leaves behind      : f32x4 acc[MI][NI], complete and safe to read
  constexpr int S = KLAB_GLDS_STAGES;
  static_assert(S == 4, "the steady-state loop is unrolled over a 4-stage ring");
  constexpr int ABYTES = OA::BYTES, STAGE = OA::BYTES + OB::BYTES;
  constexpr int LPS = OA::L + OB::L;                    // LDS-DMA instructions per wave per stage
  constexpr int NRA = MI * OA::RPF, NRB = NI * OB::RPF;  // LDS read instructions per wave per k-tile
  constexpr int NMMA = MI * NI, NOTH = NRA + NRB + LPS;
  // k-tiles are visited in a per-workgroup rotated order: workgroups that share an A or B panel start together,
  // and in lockstep they would all hit the same few L2 channels at once; rotating by the tile coordinates spreads
  // each panel's readers over its whole K extent (only the fp32 summation order changes).
  const int skew = ((bm0 / BM) * 5 + (bn0 / BN) * 3) % nt;
  auto ktile = [&](int t) { int kk = t + skew; return kt0 + (kk >= nt ? kk - nt : kk); };
  // LDS address of ring slot SN for ds_read = base register KLAB_SB(SN) + immediate KLAB_SO(SN); the immediates are 16 bits
#if KLAB_RING_TWO_BASES  // a 96 KB ring: stages 0-1 are addressed from sb0, stages 2-3 from sb1
  static_assert(2 * STAGE + 8192 <= 65536, "immediate LDS offsets: two stages per base register");
  const unsigned sb0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem, sb1 = sb0 + 2 * STAGE;
#define KLAB_SB(SN) (((SN) >> 1) ? sb1 : sb0)
#define KLAB_SO(SN) (((SN) & 1) * STAGE)
#else
  static_assert(S * STAGE <= 65536, "immediate LDS offsets");
  const unsigned sb0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
#define KLAB_SB(SN) sb0
#define KLAB_SO(SN) ((SN) * STAGE)
#endif

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 a0[MI], b0[NI], a1[MI], b1[NI];

  // "other" operation o of a step: first the LDS reads of the next k-tile (early, so they have the rest of the step to
  // land), then the LDS-DMA instructions.  SN = ring slot of the k-tile being read, SD = slot being refilled.
#define KLAB_OTHER(O, SN, SD, NA, NB, DO_DMA, KT)                                                          \
  if constexpr ((O) < NRA) oa.template read1<(O), KLAB_SO(SN)>(KLAB_SB(SN), NA);                           \
  else if constexpr ((O) < NRA + NRB) ob.template read1<(O) - NRA, KLAB_SO(SN) + ABYTES>(KLAB_SB(SN), NB);  \
  else if (DO_DMA) {                                                                                       \
    constexpr int d = (O) - NRA - NRB;                                                                     \
    if constexpr (d < OA::L) oa.issue1(d, KT, smem + (SD) * STAGE, wave);                                  \
    else ob.issue1(d - OA::L, KT, smem + (SD) * STAGE + ABYTES, wave);                                     \
  }
  // MFMAs of the current fragments (CA, CB) with the other operations spread between them
  auto mma_and = [&](auto sn_c, auto sd_c, const u32x4 (&ca)[MI], const u32x4 (&cb)[NI], u32x4 (&na)[MI], u32x4 (&nb)[NI],
                     bool do_read, bool do_dma, int kt) {
    constexpr int SN = decltype(sn_c)::value, SD = decltype(sd_c)::value;
    auto other = [&](auto oc) {
      constexpr int O = decltype(oc)::value;
      if constexpr (O < NRA + NRB) { if (do_read) { KLAB_OTHER(O, SN, SD, na, nb, false, kt) } }
      else { KLAB_OTHER(O, SN, SD, na, nb, do_dma, kt) }
    };
    auto unroll_other = [&](auto kc) {  // operations [k*NOTH/NMMA, (k+1)*NOTH/NMMA)
      constexpr int k = decltype(kc)::value, lo = k * NOTH / NMMA, hi = (k + 1) * NOTH / NMMA;
      if constexpr (hi - lo > 0) other(std::integral_constant<int, lo>{});
      if constexpr (hi - lo > 1) other(std::integral_constant<int, lo + 1>{});
      if constexpr (hi - lo > 2) other(std::integral_constant<int, lo + 2>{});
      if constexpr (hi - lo > 3) other(std::integral_constant<int, lo + 3>{});
      static_assert(hi - lo <= 4, "at most four slotted operations per MFMA gap");
    };
    auto one = [&](auto kc) {
      constexpr int k = decltype(kc)::value, i = k / NI, j = k % NI;
      KLAB_RING_MMA(acc[i][j], ca[i], cb[j])
      unroll_other(kc);
    };
    [&]<int... Ks>(std::integer_sequence<int, Ks...>) { (one(std::integral_constant<int, Ks>{}), ...); }(std::make_integer_sequence<int, NMMA>{});
  };

  // prologue: k-tiles 0 .. S-1 fill the whole ring, the fragments of k-tile 0 come in
#pragma unroll
  for (int t = 0; t < S; ++t)
    if (t < nt) {
#pragma unroll
      for (int d = 0; d < OA::L; ++d) oa.issue1(d, ktile(t), smem + t * STAGE, wave);
#pragma unroll
      for (int d = 0; d < OB::L; ++d) ob.issue1(d, ktile(t), smem + t * STAGE + ABYTES, wave);
    }
  wait_groups<LPS>((nt < S ? nt : S) - 1);  // k-tile 0 has landed
  __builtin_amdgcn_s_barrier();
  [&]<int... Rs>(std::integer_sequence<int, Rs...>) { (oa.template read1<Rs, 0>(sb0, a0), ...); }(std::make_integer_sequence<int, NRA>{});
  [&]<int... Rs>(std::integer_sequence<int, Rs...>) { (ob.template read1<Rs, ABYTES>(sb0, b0), ...); }(std::make_integer_sequence<int, NRB>{});

  int t = 0;
  // one pipeline step on k-tile t held in (CA, CB) = ring slot SC: once every wave has its fragments of t in registers
  // (lgkmcnt + barrier) slot SC is refilled with k-tile t+S, while k-tile t+1 (slot SC+1) is read into (NA, NB)
#define KLAB_STEP(SC, CA, CB, NA, NB)                                                                                  \
  {                                                                                                                   \
    wait_lgkmcnt<0>();              /* fragments of k-tile t (issued one step ago) */                                  \
    wait_vmcnt<(S - 2) * LPS>();    /* k-tile t+1 landed; S-2 younger groups stay in flight */                         \
    __builtin_amdgcn_s_barrier();   /* t+1 visible to all waves; all waves hold k-tile t in registers: slot SC is free */ \
    mma_and(std::integral_constant<int, ((SC) + 1) % S>{}, std::integral_constant<int, (SC)>{}, CA, CB, NA, NB, true, true, ktile(t + S)); \
    ++t;                                                                                                              \
  }
  while (t + S + 3 < nt) {  // four straight-line steps: every step still has a k-tile to issue
    KLAB_STEP(0, a0, b0, a1, b1)
    KLAB_STEP(1, a1, b1, a0, b0)
    KLAB_STEP(2, a0, b0, a1, b1)
    KLAB_STEP(3, a1, b1, a0, b0)
  }
#undef KLAB_STEP
  // Tail (t is a multiple of S; at most S+3 k-tiles): not pipelined.  Each step reads its own fragments into (a1, b1)
  // and consumes them at once, so no asm-loaded register is live across a branch: hipcc copies such values at control
  // flow merges, and a copy placed right behind the asm ds_read would pick the register up before the data lands.
  auto mma_plain = [&](const u32x4 (&ca)[MI], const u32x4 (&cb)[NI]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        KLAB_RING_MMA(acc[i][j], ca[i], cb[j])
      }
  };
#define KLAB_TAIL(SC, FIRST)                                                                                              \
  {                                                                                                                     \
    if constexpr (!(FIRST)) {                                                                                           \
      const int rem = nt - 1 - t;                                                                                       \
      wait_groups<LPS>(rem < S - 1 ? rem : S - 1); /* k-tile t landed */                                                 \
      __builtin_amdgcn_s_barrier();               /* ... for every wave */                                              \
      [&]<int... Rs>(std::integer_sequence<int, Rs...>) { (oa.template read1<Rs, KLAB_SO(SC)>(KLAB_SB(SC), a1), ...); }(std::make_integer_sequence<int, NRA>{});          \
      [&]<int... Rs>(std::integer_sequence<int, Rs...>) { (ob.template read1<Rs, KLAB_SO(SC) + ABYTES>(KLAB_SB(SC), b1), ...); }(std::make_integer_sequence<int, NRB>{}); \
    }                                                                                                                   \
    wait_lgkmcnt<0>();                                                                                                  \
    if (t + S < nt) {                                                                                                   \
      __builtin_amdgcn_s_barrier(); /* every wave holds k-tile t in registers: slot SC is free */                        \
      _Pragma("unroll") for (int d = 0; d < OA::L; ++d) oa.issue1(d, ktile(t + S), smem + (SC) * STAGE, wave);           \
      _Pragma("unroll") for (int d = 0; d < OB::L; ++d) ob.issue1(d, ktile(t + S), smem + (SC) * STAGE + ABYTES, wave);  \
    }                                                                                                                   \
    if constexpr (FIRST) mma_plain(a0, b0); /* prefetched by the prologue or by the last steady step */                  \
    else mma_plain(a1, b1);                                                                                             \
    ++t;                                                                                                                \
  }
#define KLAB_GENERAL_TAIL       \
  KLAB_TAIL(0, true)            \
  while (t < nt) {              \
    KLAB_TAIL(1, false)         \
    if (t >= nt) break;         \
    KLAB_TAIL(2, false)         \
    if (t >= nt) break;         \
    KLAB_TAIL(3, false)         \
    if (t >= nt) break;         \
    KLAB_TAIL(0, false)         \
  }
#if KLAB_RING_DRAIN4
  // Exactly four k-tiles left, all of them already issued (K a multiple of 128 -- every T5 / Swin width): they drain through the
  // same pipelined step as the steady state, without the DMA slot (the general tail reads each tile's fragments and waits
  // for them before its MFMAs: three exposed LDS round trips per tile of C).  The fragments of k-tile t are waited for BEFORE the
  // branch, so that a register copy hipcc may place at the branch cannot pick up data that has not landed.
  wait_lgkmcnt<0>();
  if (nt - t == 4) {
    wait_vmcnt<2 * LPS>();
    __builtin_amdgcn_s_barrier();
    mma_and(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, a0, b0, a1, b1, true, false, 0);
    wait_lgkmcnt<0>();
    wait_vmcnt<LPS>();
    __builtin_amdgcn_s_barrier();
    mma_and(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, a1, b1, a0, b0, true, false, 0);
    wait_lgkmcnt<0>();
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    mma_and(std::integral_constant<int, 3>{}, std::integral_constant<int, 2>{}, a0, b0, a1, b1, true, false, 0);
    wait_lgkmcnt<0>();
    mma_plain(a1, b1);
    t += 4;
    // the accumulators must not be touched before the last MFMA has retired (no interlock for inline-asm MFMAs), and hipcc places
    // register copies at the join of the two branches: the nops go INSIDE each branch (found the hard way: the last k-tile of
    // every product was lost)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  } else {
    KLAB_GENERAL_TAIL
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  }
#else
  KLAB_GENERAL_TAIL
#endif
#undef KLAB_GENERAL_TAIL
#undef KLAB_TAIL
#undef KLAB_OTHER
#undef KLAB_SB
#undef KLAB_SO
  // MFMA results are not interlocked against the v_accvgpr_read of the epilogue when the MFMA is inline asm
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  wait_vmcnt<0>();
#undef KLAB_RING_MMA
#undef KLAB_RING_TWO_BASES
#undef KLAB_RING_DRAIN4
