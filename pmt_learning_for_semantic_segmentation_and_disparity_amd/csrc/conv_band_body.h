// The body of conv_band_kernel and conv_band_bx_kernel (conv_band.h), which includes this file once inside each of them: the two
// kernels differ in their argument block `p` (BandArgs / BandBxArgs) alone.  Written once and compiled twice, not a function
// both call: through a function's parameter hipcc no longer reads `p` as the kernel's own argument segment and the plain
// kernels come out different (and no faster) — with the text in the kernel they are, instruction for instruction, what they
// were before the second kernel existed (tools/kernel_identity.py).  Uses the template parameters K, BN, VAR, NW, KD and `p`.
// No include guard, on purpose.
  constexpr bool DBG = (VAR & 128) != 0;                  // diagnostic build: honours p.dbg (timing breakdowns, wrong results)
  constexpr bool BX = (VAR & 8) != 0;                     // BatchNorm-backward sums in the epilogue (Args = BandBxArgs; host: 2-D, statistics on, no bias / activation)
  static_assert(!BX || (KD == 1 && !DBG), "the BatchNorm-backward epilogue: 2-D form only");
  const std::conditional_t<BX, BandBxArgs, BandArgs>& pbx = p;   // the BX fields, named only where BX holds (a type that depends on VAR: the plain kernel never looks them up)
  const int dbg = DBG ? p.dbg : 0;
  using C = BandCfg<K, BN, NW, KD>;
  using T = bf16_t;
  constexpr int IWp = C::IWp, IW = C::IW, HB = C::HB, WB = C::WB, RPR = C::RPR, RPW = C::RPW;
  constexpr int NT_CO = BN / 16, NT_PIX = 2 * RPW;
  constexpr int NSTORE = NT_CO * NT_PIX / 2;             // global stores per lane of an interior tile's epilogue
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;

  const int t_begin = blockIdx.x * p.tpw;
  const int t_end = min(p.ntiles, t_begin + p.tpw);
  if (t_begin >= t_end) return;                          // (host launches no such workgroup)
  const int nhalf = KD > 1 ? KD : (p.Cin > 32 ? 2 : 1);   // chunks per tile: channel halves, or (volumes, <= 32 channels) depth taps
  const int nchunks = (t_end - t_begin) * nhalf;

  // ---- LDS-DMA source side ----
  // lane tid fills physical 16-byte slot (tid & 3) of row round*128 + (tid >> 2); it fetches the logical chunk
  // slot ^ key(row), key = bit 2 of the row -> bit 1 of the slot (LdsRow<1>), the same in every round (128 % 8 == 0)
  const int rsub = tid >> 2;
  const int c_l = (tid & 3) ^ ((rsub >> 1) & 2);
  const unsigned wave_lds = __builtin_amdgcn_readfirstlane(lds_addr(smem) + wave * 1024);
  const band_rsrc_t xr = band_rsrc(p.x), wr = band_rsrc(p.wp);
  const int img_bytes = p.H * p.W * p.ldx * 2;

  // volumes: z runs fastest, so that a workgroup walks its spatial tile through consecutive output slices and finds two of the
  // three input slices of a tile in its XCD's L2 (it loaded them for the tile before); b counts batch entries, zt is the slice
  int czt = 0;                                            // output slice of the tile decoded last
  auto tile_of = [&](int t, int& b, int& oh0, int& ow0) {
    if constexpr (KD > 1) { const int q = fast_div(t, p.Do, p.magic_do); czt = t - q * p.Do; t = q; }
    b = fast_div(t, p.tiles_hw, p.magic_hw);
    const int r = t - b * p.tiles_hw;
    const int ty = fast_div(r, p.tiles_w, p.magic_tw);
    oh0 = ty * C::TH;
    ow0 = (r - ty * p.tiles_w) * C::TW;
  };
  // byte offsets (inside one image, channel half 0) of this lane's piece of every halo round of a tile
  int hv[C::HR];
  auto halo_offsets = [&](int oh0, int ow0) {
    const int ih0 = oh0 - p.pad_t, iw0 = ow0 - p.pad_l;
#pragma unroll
    for (int r = 0; r < C::HR; ++r) {
      const int row = r * RPR + rsub;
      const int ih = row / IWp, iw = row - ih * IWp;
      const int gh = ih0 + ih, gw = iw0 + iw;
      const bool in = iw < IW && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W && c_l * 8 < p.Cin;
      hv[r] = in ? ((gh * p.W + gw) * p.ldx + c_l * 8) * 2 : kBandOob;
    }
  };
  auto halo_dma = [&](int r, int soff, int hsel) {         // round r of the image at byte offset soff (< 0: a slice outside the volume, zeros) into halo buffer hsel
    if (r < C::HR && r * RPR + wave * 16 < C::HROWS) band_dma(soff >= 0 ? hv[r] : kBandOob, xr, hsel * HB + r * (RPR * 64) + wave_lds, soff >= 0 ? soff : 0);   // wave-uniform
  };
  // byte offset of the image a chunk reads: (batch entry / image b, chunk h of output slice zt)
  auto chunk_src = [&](int b, int zt, int h) -> int {
    if constexpr (KD > 1) {
      const int zin = zt + h - p.pad_d;
      return (zin >= 0 && zin < p.D) ? (b * p.D + zin) * img_bytes : -1;
    } else {
      return b * img_bytes + h * 64;
    }
  };
  // weights: row tap*BN + m of a stage <- row (j*K + tap)*Mpad + m of the packed [T][Mpad][64] image
  int wv[C::WR];
#pragma unroll
  for (int r = 0; r < C::WR; ++r) {
    const int row = r * RPR + rsub;
    const int tap = row / BN, m = min(row % BN, p.Mpad - 1);
    wv[r] = (tap * p.Mpad + m) * 128 + c_l * 16;
  }
  const int wrow_bytes = C::TPS * p.Mpad * 128;            // one stage (RS kernel rows) of the packed image
  auto w_dma = [&](int r, int j, int h, int wsel) {         // stage j of chunk h: channel half h (+64 bytes in the packed row) or depth tap h (its own 3x3 image)
    if (r < C::WR && r * RPR + wave * 16 < C::WROWS)
      band_dma(wv[r], wr, 2 * HB + wsel * WB + r * (RPR * 64) + wave_lds, j * wrow_bytes + (KD > 1 ? h * wrow_bytes : h * 64));
  };

  // ---- fragment addressing ----
  int b_k[K];                                             // halo byte offset of (row kw + l15, logical chunk lg)
#pragma unroll
  for (int kw = 0; kw < K; ++kw) b_k[kw] = LdsRow<1>::off(kw + l15, lg);
  const int a_base = LdsRow<1>::off(l15, lg);             // weight row l15 (+ tap*BN + mi*16 rows: key unchanged)
  const int wave_row = wave * (RPW * IWp * 64);

  float bv[NT_CO][4];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = mi * 16 + 4 * lg + r;
      bv[mi][r] = (!BX && p.bias && co < p.Cout) ? p.bias[co] : 0.f;
    }

  f32x4 acc[NT_CO][NT_PIX];
  float s1[NT_CO][4], s2[NT_CO][4];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[mi][r] = 0.f; s2[mi][r] = 0.f; }

  float* const red = reinterpret_cast<float*>(smem + 2 * HB + C::NWB * WB);
  // BX: the kernel has no registers left to carry 2 * BN / 4 sums per lane from tile to tile next to the operands issued ahead, so
  // s1 / s2 live for one epilogue only: bx_fold adds the wave's sums of a tile into ITS slots of `red` (no other wave touches them
  // between two flushes), and flush_stats only adds the waves up and clears the slots.  Behind `red`: scale and shift of the
  // current statistics group, [2][BN] floats (zero beyond Cout), rewritten behind the flush's barrier when the group changes
  float* const bxs = red + NW * 2 * BN;
  auto bx_scale = [&](int grp) {
    if constexpr (BX) {
      if (tid < 2 * BN) {
        const int which = tid / BN, m = tid - which * BN;
        bxs[tid] = m < p.Cout ? (which ? pbx.bsh : pbx.bsc)[(long)grp * p.Cout + m] : 0.f;
      }
    }
  };
  auto bx_fold = [&]() {
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = row16_sum(s1[mi][r]), c2 = row16_sum(s2[mi][r]);
        if (l15 == 0) {
          const int m = mi * 16 + 4 * lg + r;
          red[(wave * 2 + 0) * BN + m] += a;
          red[(wave * 2 + 1) * BN + m] += c2;
        }
      }
  };
  auto flush_stats = [&](int grp) {                        // every wave; ends with the sums of `grp` added to p.stats
    if constexpr (!BX) {
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = row16_sum(s1[mi][r]), c2 = row16_sum(s2[mi][r]);
          if (l15 == 0) {
            const int m = mi * 16 + 4 * lg + r;
            red[(wave * 2 + 0) * BN + m] = a;
            red[(wave * 2 + 1) * BN + m] = c2;
          }
          s1[mi][r] = 0.f; s2[mi][r] = 0.f;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (tid < 2 * BN) {
      const int which = tid / BN, m = tid - which * BN;
      if (m < p.Cout) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += red[(w * 2 + which) * BN + m];
        if constexpr (BX) {
#pragma unroll
          for (int w = 0; w < NW; ++w) red[(w * 2 + which) * BN + m] = 0.f;   // (its wave adds to it again behind the next stage's barrier)
        }
        atomicAdd(p.stats + (long)(blockIdx.x % p.nrep) * p.rep_stride + ((long)grp * 2 + which) * p.stats_ld + m, (double)tot);
      }
    }
  };

  if constexpr ((VAR & 2) != 0) { if (wave >= 4) __builtin_amdgcn_s_setprio(1); }
  // ---- prime: the weights of the first kernel row, then the halo of chunk 0 ----
  int cb, coh0, cow0, ch_half = 0, ct = t_begin;           // current chunk: image, tile origin, channel half, tile
  tile_of(ct, cb, coh0, cow0);
  if constexpr (BX) {   // in front of the first DMA (the compiler waits for these loads with vmcnt(0)); published by the first stage's barrier
    for (int i = lane; i < 2 * BN; i += 64) red[wave * 2 * BN + i] = 0.f;
    bx_scale(cb < p.bpg ? 0 : cb / p.bpg);
  }
  halo_offsets(coh0, cow0);
#pragma unroll
  for (int r = 0; r < C::WR; ++r) w_dma(r, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < C::HR; ++r) halo_dma(r, chunk_src(cb, czt, 0), 0);
  int cz = czt;                                            // output slice of the current tile
  int wsel = 0;
  bool epi_counted = false;                                // the previous chunk ended with exactly NSTORE stores per lane

  // 3x3, <= 32 output channels: the resident weights (9 taps x 2 fragments) stay in REGISTERS — every tile uses the same ones, and with
  // two output-channel tiles per wave the weight fragments were a third of the kernel's LDS reads, which bound it (6 reads per 8 MFMAs)
  constexpr bool WREG = C::WRES && BN <= 32;
  u32x4 wreg[WREG ? C::TPS : 1][NT_CO];
  constexpr bool BXR = (VAR & 16) != 0;                    // BX with an addend (host: p.res set) — a flag, not a branch: a uniform branch per store cost the 64-channel forms ~120 spilled registers
  constexpr int BXQA = BX && BN <= 32 ? NT_PIX / 2 : 0;   // pixel rows of u issued a stage ahead (below): what the registers allow
  constexpr bool BXRA = BXR && K == 5 && BN <= 32;         // ... and the addend with them

  for (int c = 0; c < nchunks; ++c) {
    const int hsel = c & 1;
    const bool has_next = c + 1 < nchunks;
    // next chunk
    int nb = cb, noh0 = coh0, now0 = cow0, nh = ch_half + 1, nt = ct, nz = cz;
    if (nh == nhalf) {
      nh = 0; nt = ct + 1;
      if (has_next) { tile_of(nt, nb, noh0, now0); halo_offsets(noh0, now0); nz = czt; }
    }
    const int nsoff = chunk_src(nb, nz, nh);
    if (ch_half == 0) {
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const unsigned char* const hb = smem + hsel * HB + wave_row;

    // BX: the u operands of an interior tile, in exactly the layout of the 16-byte stores, are — at 32 output channels (BXQA) —
    // issued at the start of the tile's LAST stage and used only in the epilogue, a stage (~2 us) later.  Ordinary loads: the compiler waits for them (and, vmcnt
    // retiring in order, for the weight / halo DMA issued behind them) at their first use, which is where stage 0 of the next
    // chunk waits anyway.  Nothing is issued between two points a counted band_wait<N> spans: the loads go out right behind the
    // stage's barrier, in front of its first DMA, and the stage that follows waits on the epilogue's stores alone (or on everything).
    // The addend goes with them where the registers allow it (BXRA: 5x5 with 32 output channels).  The 64-channel forms stand
    // at 248 of 256 registers in the stage loop without either, so there u — and, where it is not ahead, the addend — is issued
    // in one batch at the head of the epilogue, where the fragment registers are free: one exposed round trip per tile
    // instead of one per pixel row.
    // (declared per chunk: a value defined and used under the same condition must not look loop-carried, or it holds its registers through every stage)
    u32x4 bxu[BX ? NT_PIX / 2 : 1][NT_CO], bxr[BXR ? NT_PIX / 2 : 1][NT_CO];
    auto bx_issue = [&](bool with_u, bool with_res, int q0, int q1) {   // pixel rows q0 .. q1 - 1 of the wave (constants at every call)
      if constexpr (BX) {
        if (!(coh0 + C::TH <= p.Ho && cow0 + C::TW <= p.Wo && BN <= p.Cout)) return;   // workgroup-uniform: ragged tiles load in the epilogue, guarded
        const long pix0 = ((long)cb * p.Ho + coh0 + RPW * wave) * p.Wo + cow0 + (lg & 1) * 16 + l15;
        if (with_u) {
          const T* const u0 = (const T*)pbx.bx + pix0 * pbx.ldbx + 8 * (lg >> 1);
#pragma unroll
          for (int q = 0; q < NT_PIX / 2; ++q)
#pragma unroll
            for (int mi = 0; mi < NT_CO; ++mi) if (q >= q0 && q < q1) bxu[q][mi] = *reinterpret_cast<const u32x4*>(u0 + (long)q * p.Wo * pbx.ldbx + mi * 16);
        }
        if constexpr (BXR) {
          if (with_res) {
            const T* const r0 = (const T*)p.res + pix0 * p.ldres + 8 * (lg >> 1);
#pragma unroll
            for (int q = 0; q < NT_PIX / 2; ++q)
#pragma unroll
              for (int mi = 0; mi < NT_CO; ++mi) if (q >= q0 && q < q1) bxr[q][mi] = *reinterpret_cast<const u32x4*>(r0 + (long)q * p.Wo * p.ldres + mi * 16);
          }
        }
      }
    };

    band_static_for<0, C::NSTG>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      // The weights of this stage (and, entering stage 0, the whole halo image) have landed once at most the operations
      // issued behind them are outstanding: the halo rounds of the previous stage (counted only where every wave issued
      // the same number), or the previous tile's epilogue stores (vmcnt retires in issue order).
      constexpr int r_lo = (j - 1) * C::HPS, r_hi = j * C::HPS < C::HR ? j * C::HPS : C::HR;
      constexpr bool counted = j >= 1 && r_hi > r_lo && r_hi * RPR <= C::HROWS;
      if (j == 0 && epi_counted) band_wait<NSTORE>();
      else if (counted && has_next) band_wait<counted ? r_hi - r_lo : 0>();
      else band_wait<0>();
      if (!(dbg & 16)) __builtin_amdgcn_s_barrier();

      const unsigned char* const wl = smem + 2 * HB + wsel * WB + a_base;
      const unsigned char* const hj = hb + j * C::RS * (IWp * 64);
      if constexpr (WREG) {
        if (c == 0) {                                       // (the weights landed with the first image: the wait above)
#pragma unroll
          for (int t = 0; t < C::TPS; ++t)
#pragma unroll
            for (int mi = 0; mi < NT_CO; ++mi) wreg[t][mi] = *reinterpret_cast<const u32x4*>(wl + t * (BN * 64) + mi * 1024);
        }
      }
      if constexpr (BXQA > 0 && j == C::NSTG - 1) { if (ch_half == nhalf - 1) bx_issue(true, BXRA, 0, BXQA); }   // the tile's last stage
      u32x4 af[2][NT_CO], bf[2][NT_PIX];
      if constexpr (DBG) if (dbg & 32) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) { if (q < NT_CO) af[i][q] = u32x4{0x3f803f80u, (unsigned)tid, 0x3f803f80u, 0x3f803f80u}; bf[i][q] = u32x4{0x3f803f80u, 0x3f803f80u, (unsigned)lane, 0x3f803f80u}; }
      }
      auto load = [&](int set, int t) {                     // tap t of the stage: kernel row t / K of it, column t % K
        if (dbg & 32) return;
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi) {
          if constexpr (WREG) af[set][mi] = wreg[t][mi];
          else af[set][mi] = *reinterpret_cast<const u32x4*>(wl + t * (BN * 64) + mi * 1024);
        }
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni)
          bf[set][ni] = *reinterpret_cast<const u32x4*>(hj + b_k[t % K] + ((t / K + (ni >> 1)) * IWp + (ni & 1) * 16) * 64);
      };
      // DMA slot s of the stage, issued between the fragment reads of tap s+1 and the MFMAs of tap s: first the weights
      // of the next stage, behind them this stage's share of the next chunk's halo
      auto dma_slot = [&](int sl) {
        if (sl < C::WRS) {
          if (dbg & 2) return;
          if (j + 1 < C::NSTG) w_dma(sl, j + 1, ch_half, wsel ^ 1);
          else if (has_next) w_dma(sl, 0, nh, wsel ^ 1);
        } else if (sl < C::WRS + C::HPS) {
          if (dbg & 1) return;
          if (has_next && (C::NSTG == 1 || j < C::NSTG - 1)) halo_dma(j * C::HPS + sl - C::WRS, nsoff, hsel ^ 1);
        }
      };
      load(0, 0);
#pragma unroll
      for (int kw = 0; kw < C::TPS; ++kw) {                 // (kw: tap index inside the stage)
        if constexpr ((VAR & 1) != 0) {
#pragma unroll
          for (int sl = kw * C::SPT; sl < (kw + 1) * C::SPT; ++sl) dma_slot(sl);
        }
        if (kw + 1 < C::TPS) load((kw + 1) & 1, kw + 1);
        if constexpr ((VAR & 1) == 0) {
#pragma unroll
          for (int sl = kw * C::SPT; sl < (kw + 1) * C::SPT; ++sl) dma_slot(sl);
        }
        if (!(dbg & 4)) {
#pragma unroll
          for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
            for (int ni = 0; ni < NT_PIX; ++ni) Mma<T>::run(acc[mi][ni], af[kw & 1][mi], bf[kw & 1][ni]);
        }
        if constexpr ((VAR & 4) != 0) {                    // one fragment read per two MFMAs
#pragma unroll
          for (int g = 0; g < NT_CO + NT_PIX; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, (NT_CO * NT_PIX) / (NT_CO + NT_PIX), 0);
          }
        }
      }
      if constexpr (!C::WRES) wsel ^= 1;
    });

    epi_counted = false;
    if (ch_half == nhalf - 1) {
      // ---- epilogue of tile ct: bias / activation / store / BatchNorm statistics of the stored values ----
      const int oimg = KD > 1 ? cb * p.Do + cz : cb;        // output image (slice)
      const int grp = oimg < p.bpg ? 0 : oimg / p.bpg;
      if constexpr (BX) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r) { s1[mi][r] = 0.f; s2[mi][r] = 0.f; }
      }
      if (!BX && p.bias) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][ni][r] += bv[mi][r];
      }
      if (!BX && p.act == 1) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][ni][r] = fmaxf(acc[mi][ni][r], 0.f);
      } else if (!BX && p.act == 2) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][ni][r] = 1.f / (1.f + __expf(-acc[mi][ni][r]));
      }
      T* const yb = (T*)p.y + (long)oimg * p.Ho * p.Wo * p.ldy;
      const T* const rb = (const T*)p.res + (long)oimg * p.Ho * p.Wo * p.ldres;
      const bool interior = coh0 + C::TH <= p.Ho && cow0 + C::TW <= p.Wo && BN <= p.Cout;   // workgroup-uniform
      if (interior) {
        // 16-byte stores: v_permlane16_swap trades the 4 channels a lane holds for pixel tile 2q+1 against the NEXT 4
        // channels (lane + 16) of pixel tile 2q, so that lane rows 0/2 own 8 consecutive channels of tile 2q and rows
        // 1/3 of tile 2q+1: half the store instructions of the 8-byte form, the cost that bounds the epilogue
        const long pix0 = (long)(coh0 + RPW * wave) * p.Wo + cow0 + (lg & 1) * 16 + l15;   // this lane's pixel of row q = 0 after the swap
        T* const d0 = yb + pix0 * p.ldy + 8 * (lg >> 1);
        const T* const r0 = rb + pix0 * p.ldres + 8 * (lg >> 1);
        if constexpr (BX) {   // what did not go out ahead: all of it at once, in front of the first use
          if constexpr (BXQA < NT_PIX / 2) bx_issue(true, false, BXQA, NT_PIX / 2);
          if constexpr (BXR && !BXRA) bx_issue(false, true, 0, NT_PIX / 2);
        }
        if constexpr (BX) {   // the operands' first use is HERE: nothing derived from u (the mask needs no accumulator) may move up into the MFMA loop
#pragma unroll
          for (int q = 0; q < NT_PIX / 2; ++q)
#pragma unroll
            for (int mi = 0; mi < NT_CO; ++mi) asm volatile("" : "+v"(bxu[q][mi]));
        }
        // q outside, mi inside: the four 32-byte pieces of a pixel's 128-byte line leave in four CONSECUTIVE store
        // instructions and merge in L2 (with mi outside, WRITE_SIZE read 1.8x the output: partial lines written back)
#pragma unroll
        for (int q = 0; q < NT_PIX / 2; ++q) {               // pixel tiles 2q, 2q+1: the two 16-pixel halves of one row
          T* dst = d0 + (long)q * p.Wo * p.ldy;
          const T* rsrc = r0 + (long)q * p.Wo * p.ldres;
          u32x4 ov[NT_CO];
#pragma unroll
          for (int mi = 0; mi < NT_CO; ++mi) {
            const f32x4 v0 = acc[mi][2 * q], v1 = acc[mi][2 * q + 1];
            if constexpr (BX) {
              // u and the addend arrive in the store layout; the same swap that makes it takes them back to the accumulator
              // layout (it is its own inverse: dwords 0 / 2 hold channels r = 0, 1 of tiles 2q / 2q+1, dwords 1 / 3 r = 2, 3).
              // There the sum is formed (f32, rounded once — the arithmetic of the plain addend form), masked and added up.
              const u32x4 ub = bxu[q][mi];
              const u32x2 ua = __builtin_amdgcn_permlane16_swap(ub[0], ub[2], false, false);
              const u32x2 uc = __builtin_amdgcn_permlane16_swap(ub[1], ub[3], false, false);
              const unsigned ua0 = ua[0], ua1 = ua[1], uc0 = uc[0], uc1 = uc[1];
              float f0[4], f1[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) { f0[r] = v0[r]; f1[r] = v1[r]; }
              if constexpr (BXR) {
                const u32x4 rb4 = bxr[q][mi];
                const u32x2 ra = __builtin_amdgcn_permlane16_swap(rb4[0], rb4[2], false, false);
                const u32x2 rc = __builtin_amdgcn_permlane16_swap(rb4[1], rb4[3], false, false);
                const unsigned ra0 = ra[0], ra1 = ra[1], rc0 = rc[0], rc1 = rc[1];
                f0[0] += bflo(ra0); f0[1] += bfhi(ra0); f0[2] += bflo(rc0); f0[3] += bfhi(rc0);
                f1[0] += bflo(ra1); f1[1] += bfhi(ra1); f1[2] += bflo(rc1); f1[3] += bfhi(rc1);
              }
              const unsigned p00 = pack2bf(f0[0], f0[1]), p01 = pack2bf(f0[2], f0[3]);
              const unsigned p10 = pack2bf(f1[0], f1[1]), p11 = pack2bf(f1[2], f1[3]);
              const float g0[4] = {bflo(p00), bfhi(p00), bflo(p01), bfhi(p01)}, g1[4] = {bflo(p10), bfhi(p10), bflo(p11), bfhi(p11)};
              const float u0[4] = {bflo(ua0), bfhi(ua0), bflo(uc0), bfhi(uc0)}, u1[4] = {bflo(ua1), bfhi(ua1), bflo(uc1), bfhi(uc1)};
              const f32x4 sc = *reinterpret_cast<const f32x4*>(bxs + mi * 16 + 4 * lg), sh = *reinterpret_cast<const f32x4*>(bxs + BN + mi * 16 + 4 * lg);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float scr = sc[r], shr = sh[r];
                const float gm0 = fmaf(u0[r], scr, shr) > 0.f ? g0[r] : 0.f;
                const float gm1 = fmaf(u1[r], scr, shr) > 0.f ? g1[r] : 0.f;
                s1[mi][r] = fmaf(gm1, u1[r], fmaf(gm0, u0[r], s1[mi][r]));
                s2[mi][r] += gm0 + gm1;
              }
              const u32x2 e0 = __builtin_amdgcn_permlane16_swap(p00, p10, false, false);
              const u32x2 e1 = __builtin_amdgcn_permlane16_swap(p01, p11, false, false);
              ov[mi] = u32x4{e0[0], e1[0], e0[1], e1[1]};
              continue;
            }
            const u32x2 o0 = u32x2{pack2bf(v0[0], v0[1]), pack2bf(v0[2], v0[3])};
            const u32x2 o1 = u32x2{pack2bf(v1[0], v1[1]), pack2bf(v1[2], v1[3])};
            if (p.stats) {
              const f32x4 w0 = f32x4{bflo(o0[0]), bfhi(o0[0]), bflo(o0[1]), bfhi(o0[1])};
              const f32x4 w1 = f32x4{bflo(o1[0]), bfhi(o1[0]), bflo(o1[1]), bfhi(o1[1])};
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                s1[mi][r] += w0[r] + w1[r];
                s2[mi][r] = fmaf(w1[r], w1[r], fmaf(w0[r], w0[r], s2[mi][r]));
              }
            }
            u32x4 o;
            if (p.res) {                                     // uniform: y = result + res, summed in f32 and rounded once
              float f[8];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                // (scalars first: __builtin_bit_cast on a vector ELEMENT reads element 0 under hipcc 7.2, see sdhip_common.h)
                const float a0 = v0[r], a1 = v1[r];
                const u32x2 e = __builtin_amdgcn_permlane16_swap(__float_as_uint(a0), __float_as_uint(a1), false, false);
                const unsigned e0 = e[0], e1 = e[1];
                f[r] = __uint_as_float(e0); f[4 + r] = __uint_as_float(e1);
              }
              const u32x4 old = *reinterpret_cast<const u32x4*>(rsrc + mi * 16);
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = pack2bf(f[2 * e] + bflo(old[e]), f[2 * e + 1] + bfhi(old[e]));
            } else {
              const u32x2 e0 = __builtin_amdgcn_permlane16_swap(o0[0], o1[0], false, false);
              const u32x2 e1 = __builtin_amdgcn_permlane16_swap(o0[1], o1[1], false, false);
              o = u32x4{e0[0], e1[0], e0[1], e1[1]};
            }
            ov[mi] = o;
          }
          if (!(dbg & 8)) {                                  // the line's pieces back to back
#pragma unroll
            for (int mi = 0; mi < NT_CO; ++mi) *reinterpret_cast<u32x4*>(dst + mi * 16) = ov[mi];
          }
        }
        epi_counted = !(dbg & 8) && (BX || !p.res);      // (the plain form's addend loads sit among the stores; BX: every load is issued ahead or at the head of the epilogue, in front of the first store)
      } else {
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni) {
          const int oh = coh0 + RPW * wave + (ni >> 1), ow = cow0 + (ni & 1) * 16 + l15;
          const bool valid = oh < p.Ho && ow < p.Wo;
          T* dst = yb + ((long)oh * p.Wo + ow) * p.ldy;
          const T* rsrc = rb + ((long)oh * p.Wo + ow) * p.ldres;
#pragma unroll
          for (int mi = 0; mi < NT_CO; ++mi) {
            const int co = mi * 16 + 4 * lg;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[mi][ni][r];
            if (valid && co + 3 < p.Cout) {
              if (BX ? BXR : p.res != nullptr) {
                const u32x2 old = *reinterpret_cast<const u32x2*>(rsrc + co);
                v[0] += bflo(old[0]); v[1] += bfhi(old[0]); v[2] += bflo(old[1]); v[3] += bfhi(old[1]);
              }
              const u32x2 o = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
              *reinterpret_cast<u32x2*>(dst + co) = o;
              v[0] = bflo(o[0]); v[1] = bfhi(o[0]); v[2] = bflo(o[1]); v[3] = bfhi(o[1]);
            } else if (valid && co < p.Cout) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                if (co + r < p.Cout) {
                  if (BX ? BXR : p.res != nullptr) v[r] += Elem<T>::ld(rsrc + co + r);
                  Elem<T>::st(dst + co + r, v[r]); v[r] = Elem<T>::rnd(v[r]);
                }
                else v[r] = 0.f;
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = 0.f;
            }
            if constexpr (BX) {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[mi][ni][r] = v[r];   // the stored value, 0 outside the result: for the pass below
            } else if (p.stats) {
#pragma unroll
              for (int r = 0; r < 4; ++r) { s1[mi][r] += v[r]; s2[mi][r] = fmaf(v[r], v[r], s2[mi][r]); }
            }
          }
        }
        if constexpr (BX) {
          // ragged tile / channel tail: the sums in a pass of their own behind the stores (in one pass with them the 64-channel
          // forms spill).  u is loaded without a branch, from the pixel and the 4-channel group clamped into the map (host:
          // Cout % 4 == 0, so a group lies entirely inside u's channels or entirely outside) — never from outside u; a pixel
          // or channel outside the result has gm = 0 (above) and adds nothing, whatever was loaded for it
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni) {
            const int oh = min(coh0 + RPW * wave + (ni >> 1), p.Ho - 1), ow = min(cow0 + (ni & 1) * 16 + l15, p.Wo - 1);
            const T* const usrc = (const T*)pbx.bx + ((long)oimg * p.Ho * p.Wo + (long)oh * p.Wo + ow) * pbx.ldbx;
#pragma unroll
            for (int mi = 0; mi < NT_CO; ++mi) {
              const int co = mi * 16 + 4 * lg;
              const u32x2 uu = *reinterpret_cast<const u32x2*>(usrc + min(co, p.Cout - 4));
              const unsigned uu0 = uu[0], uu1 = uu[1];
              const float uf[4] = {bflo(uu0), bfhi(uu0), bflo(uu1), bfhi(uu1)};
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float g = acc[mi][ni][r];
                const float gm = fmaf(uf[r], bxs[co + r], bxs[BN + co + r]) > 0.f ? g : 0.f;
                s1[mi][r] = fmaf(gm, uf[r], s1[mi][r]); s2[mi][r] += gm;
              }
            }
          }
        }
      }
      if constexpr (BX) bx_fold();
      if (p.stats) {
        const int nimg = KD > 1 ? nb * p.Do + nz : nb;
        const int ngrp = nimg < p.bpg ? 0 : nimg / p.bpg;
        if (!has_next || ngrp != grp) {                                            // workgroup-uniform
          flush_stats(grp); epi_counted = false;
          if constexpr (BX) { if (has_next) bx_scale(ngrp); }                     // (every wave is past its epilogue: the flush's barrier)
        }
      }
    }
    cb = nb; coh0 = noh0; cow0 = now0; ch_half = nh; ct = nt; cz = nz;
  }
