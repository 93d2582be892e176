// The body of one register-resident pass over tiles (see fft_pow2_impl.h), textually included twice: into the
// stand-alone kernel fft_pow2_kernel -- where `d` IS the kernel argument: handing it to a device function by
// reference made the compiler materialise the whole descriptor up front, and the fat fp32 plans (R = 32) went
// from 124 / 126 VGPRs to 128 + 32 bytes of scratch -- and into pow2_body, the device function the fused
// kernels call.  The includer defines GFFT_TILE_LOOP (the loop header), GFFT_TILE_INDEX (`const unsigned tile
// = ...;`) and GFFT_AFTER_LOADS (a statement run once per tile behind its loads, or nothing); names in scope:
// d, in, out, smem, GFFT_SCALE (the pass's scale factor), and the template parameters real, N, R, T, COLS, SPLIT, FLAGS, MODE, BIGTW, RADS.
  static_assert(SPLIT || sizeof(real) == 4, "fp64 exchanges split planes");
  // the FLAGS bits (gfft_internal.h has the table), each decoded once
  constexpr bool NT_LD = (FLAGS & PF_NT_LOAD) != 0, NT_ST = (FLAGS & PF_NT_STORE) != 0, ACCESS_ONLY = (FLAGS & PF_ACCESS_ONLY) != 0;
  constexpr bool TRUNC = (FLAGS & PF_TRUNC) != 0, TRUNC_LOAD = (FLAGS & PF_TRUNC_LOAD) != 0, TRANSPOSE = (FLAGS & PF_TRANSPOSE_STORE) != 0;
  constexpr bool UNEVEN = (FLAGS & PF_UNEVEN_BLOCKS) != 0, NO_PIN = (FLAGS & PF_NO_PIN) != 0;
  constexpr bool SYS_ST = (FLAGS & PF_SYS_STORE) != 0, SYS_LD = (FLAGS & PF_SYS_LOAD) != 0;
  constexpr bool PLAIN = (FLAGS & PF_NATURAL) != 0, BLK_IN = (FLAGS & PF_BLOCKS_IN) != 0, BLK_OUT = (FLAGS & PF_BLOCKS_OUT) != 0;
  constexpr bool ORDER = (FLAGS & PF_ORDER) != 0;
  static_assert(!(FLAGS & (TF_NO_FOURSTEP | TF_NO_TRUNC)), "table-only bits: launch_pow2_inst strips them");
  static_assert(!TRUNC_LOAD || TRUNC, "PF_TRUNC_LOAD needs PF_TRUNC");
  static_assert(!(BLK_IN || BLK_OUT) || PLAIN, "PF_BLOCKS_IN / PF_BLOCKS_OUT need PF_NATURAL");
  // (Geo, fft_pow2_impl.h: RL / RS values per thread on the load / store side, NTL / NTS threads per column that hold them,
  // NT threads per column in the workgroup -- all of them N / R unless a stage's radix does not divide R)
  using GEO = Geo<N, R, RADS...>;
  constexpr int NT = GEO::TPC, RL = GEO::RL, RS = GEO::RS, NTL = N / RL, NTS = N / RS;
  // rows no wider than a wavefront: exchanges without barriers (tile_sync, fft_pow2_impl.h)
  constexpr bool WL = GEO::UNIFORM && WaveLocal<N, R, COLS>::value;
  constexpr int WORD = SPLIT ? sizeof(real) : 2 * sizeof(real);
  constexpr int CS = Lds<N, COLS, T, WORD == 4, FirstRadix<RADS...>::value>::CS;
  constexpr int PADSH = pad_shift<N, FirstRadix<RADS...>::value, COLS>();      // slot padding of the LDS exchanges (fft_pow2_impl.h)
  // packed-real modes move complex pairs on both sides; the Hermitian pass is in the kernel body
  constexpr bool HALF = MODE == MODE_R2C_H || MODE == MODE_C2R_H;
  constexpr int IOMODE = HALF ? MODE_C2C : MODE;
  static_assert(!HALF || (!COLS && !BIGTW && !TRANSPOSE), "packed-real modes: contiguous axis only");
  static_assert(!UNEVEN || HALF, "PF_UNEVEN_BLOCKS: packed-real rows");
  static_assert(GEO::UNIFORM || ((MODE == MODE_C2C || HALF) && !BIGTW && !(TRANSPOSE || UNEVEN)), "stages of unequal width: complex passes and packed-real rows on natural layouts (fused truncation / padding included)");
  static_assert(!(SYS_ST || SYS_LD) || ((MODE == MODE_C2C || HALF) && !(TRUNC || UNEVEN)), "hand-off buffers: plain complex passes and plain packed-real rows");
  // (PLAIN: the layout fields below are compile-time zeros; BLK_IN / BLK_OUT keep the equal blocks of the transformed axis -- the
  // step between thread slots is workgroup uniform, so the jump is scalar work.  With both kept on one pass the compiler waited
  // for every ring load before it issued the next, tools/scan_serial_loads.py: chains of 29 / 32)
  // ORDER: which thread takes which row, and from which slot q0 on a thread issues its loads and stores, follow PassDesc::order
  static_assert(!ORDER || (COLS && !BIGTW && GEO::UNIFORM && MODE == MODE_C2C && !(TRUNC || TRANSPOSE || UNEVEN || SYS_ST || SYS_LD) &&
                           (NTL & (NTL - 1)) == 0 && RL % 4 == 0 && RL == RS),
                "row orders: plain strided complex passes");
  // Conjugation-on-load applied once, BEHIND the loads, in the unequal-width stage kernels where -- applied to each value as it
  // arrives -- the compiler waited for every load before it issued the next (serial_loads_f64, fft_pow2_impl.h).  Packed-real
  // rows never conjugate on load (conj_in = 0: half_desc, plan_fused3 rows): no sign at all there.
  constexpr bool NO_SIGN = !GEO::UNIFORM && HALF && !(TRUNC_LOAD || UNEVEN || SYS_LD);
  constexpr bool DEFER_SIGN = NO_SIGN || (!GEO::UNIFORM && MODE == MODE_C2C && !(TRUNC_LOAD || UNEVEN || SYS_LD) && sizeof(real) == 8 &&
                                          serial_loads_f64(N, COLS, TRUNC));
  const auto L_in_tlg = PLAIN ? decltype(d.in_tlg)(0) : d.in_tlg;
  const auto L_out_tlg = PLAIN ? decltype(d.out_tlg)(0) : d.out_tlg;
  const auto L_in_lgp = (PLAIN && !BLK_IN) ? decltype(d.in_lgp)(0) : d.in_lgp;
  const auto L_out_lgp = (PLAIN && !BLK_OUT) ? decltype(d.out_lgp)(0) : d.out_lgp;
  const auto L_in_jump = (PLAIN && !BLK_IN) ? decltype(d.in_jump)(0) : d.in_jump;
  const auto L_out_jump = (PLAIN && !BLK_OUT) ? decltype(d.out_jump)(0) : d.out_jump;
  const auto L_in_ilg = PLAIN ? decltype(d.in_ilg)(0) : d.in_ilg;
  const auto L_out_ilg = PLAIN ? decltype(d.out_ilg)(0) : d.out_ilg;
  const auto L_fl_bw = PLAIN ? decltype(d.fl_bw)(0) : d.fl_bw;
  const auto L_flat = PLAIN ? decltype(d.flat)(0) : d.flat;
  const auto L_inner_ld = PLAIN ? decltype(d.inner_ld)(0) : d.inner_ld;
  const auto L_inner_st = PLAIN ? decltype(d.inner_st)(0) : d.inner_st;
  const auto L_out_pad = (PLAIN && !HALF) ? decltype(d.out_pad)(0) : d.out_pad;   // (packed-real rows into a hand-off slot complete its last line too)
  [[maybe_unused]] const SysBuf sys_in(in), sys_out(out);
  const cx<real> *tw = reinterpret_cast<const cx<real> *>(d.tw);
  const int tid = threadIdx.x;
  const int c = COLS ? (tid % T) : (tid / NT);
  const int t = COLS ? (tid / T) : (tid % NT);
  void *col = smem + (size_t)c * CS * WORD;
  const unsigned batch = (unsigned)d.batch, inner = (unsigned)d.inner, mid = (unsigned)d.mid;
  // COLS: a tile is T adjacent columns of ONE row of the batch (never straddles a row, so
  // segments keep their alignment when `inner` is not a multiple of T, e.g. 513-wide half
  // spectra); the (row, chunk) split is workgroup-uniform scalar arithmetic.
  // ROWS: the batch is flat (each column is itself a contiguous row of the array).
  // (four-step passes -- BIGTW -- run their columns along `mid` and use the flat form too.)
  constexpr bool ROWTILES = COLS && !BIGTW;
  const unsigned flat_cols = mid * inner;                       // L_flat: columns per outer index
  const unsigned chunks = ROWTILES ? ((L_flat ? flat_cols : inner) + T - 1) / T : 1;
  const unsigned ntiles = ROWTILES ? (L_flat ? batch / flat_cols : batch / inner) * chunks : (batch + T - 1) / T;
  const real sy_in = d.conj_in ? (real)-1 : (real)1;
  const real sx_out = (real)(MODE == MODE_R2C_H ? 0.5 * GFFT_SCALE : GFFT_SCALE);   // (the Hermitian pass leaves 2 X)
  const real sy_out = d.conj_out ? -sx_out : sx_out;
  // per thread (tile-major lines, PassDesc::in_tlg / out_tlg: tile index and lane within the tile)
  const int64_t t_in = (!COLS && L_in_tlg) ? (int64_t)(t >> L_in_tlg) * d.in_tS + (t & ((1 << L_in_tlg) - 1)) : (int64_t)t * d.in_es;
  const int64_t t_out = (!COLS && L_out_tlg) ? (int64_t)(t >> L_out_tlg) * d.out_tS + (t & ((1 << L_out_tlg) - 1)) : (int64_t)t * d.out_es;
  // fused padding / truncation: distance between the two halves of the padded spectrum (uniform)
  const int64_t pad_shift_in = TRUNC ? (int64_t)(d.n - d.tr_N) * d.in_es : 0;
  const int64_t pad_shift_out = TRUNC ? (int64_t)(d.n - d.tr_N) * d.out_es : 0;
  const int64_t q_in = (!COLS && L_in_tlg) ? (int64_t)(NTL >> L_in_tlg) * d.in_tS : (int64_t)NTL * d.in_es;     // uniform steps
  const int64_t q_out = (!COLS && L_out_tlg) ? (int64_t)(NTS >> L_out_tlg) * d.out_tS : (int64_t)NTS * d.out_es;

  GFFT_TILE_LOOP {
    GFFT_TILE_INDEX
    if (tile >= ntiles) continue;
    // The thread's row index, laundered once per tile: everything derived from it inside the loop
    // (twiddle-table offsets k*step, LDS slots, mirrored c2r offsets) is loop invariant, and
    // hoisted it sits in -- or spills from -- 2 VGPRs per use for the whole kernel.
    int tl = t;
    [[maybe_unused]] int ord_q0 = 0;      // (ORDER: the slot the tile's loads and stores start from, in quarters of RL; uniform)
    if constexpr (ORDER) {
      const unsigned rot = order_row_rot(d.order), ways = order_q0_ways(d.order);
      if (rot) tl = (int)(((unsigned)t + ord_hash * (rot == 1 ? 5u : 4u)) & (unsigned)(NTL - 1));
      ord_q0 = ways == 2 ? (int)(ord_hash & 3u) : (ways == 1 ? (int)((ord_hash & 1u) * 2u) : 0);
    }
    asm volatile("" : "+v"(tl));
    bool valid, valid_st;
    unsigned o, m, i;
    if constexpr (ROWTILES) {
      const unsigned row = tile / chunks, j = tile - row * chunks;
      if (L_flat) {
        // tiles over the flattened (m, i) index of one outer slab: per-lane row and column
        o = row;
        unsigned J = j * T + c;
        valid = valid_st = J < flat_cols;
        if (!valid) J = 0;
        m = J / inner;
        i = J - m * inner;
      } else {
        i = j * T + c;
        valid = i < (L_inner_ld ? (unsigned)L_inner_ld : inner);          // columns that are read
        valid_st = i < (L_inner_st ? (unsigned)L_inner_st : inner);       // columns that are written
        if (!(valid || valid_st)) i = 0;
        o = row / mid;
        m = row - o * mid;
      }
    } else {
      const unsigned b = tile * T + c;
      valid = valid_st = b < batch;
      const unsigned bb = valid ? b : 0;
      const unsigned bm = bb / inner;
      i = bb - bm * inner;
      o = bm / mid;
      m = bm - o * mid;
    }
    int64_t in0 = (int64_t)o * d.in_os + (int64_t)m * d.in_ms, out0 = (int64_t)o * d.out_os + (int64_t)m * d.out_ms;
    if constexpr (COLS) {
      // (tile-major columns of an exchange buffer, PassDesc::in_ilg / out_ilg; flat tiles over rows
      // stored as body + leftover columns, PassDesc::fl_bw)
      if (L_fl_bw && i >= (unsigned)L_fl_bw) in0 = (int64_t)o * d.in_os + d.fl_tail + (int64_t)m * d.fl_tail_ms + (i - (unsigned)L_fl_bw);
      else in0 += L_in_ilg ? (int64_t)(i >> L_in_ilg) * d.in_iS + (i & ((1u << L_in_ilg) - 1)) : (int64_t)i * d.in_is;
      out0 += L_out_ilg ? (int64_t)(i >> L_out_ilg) * d.out_iS + (i & ((1u << L_out_ilg) - 1)) : (int64_t)i * d.out_is;
    } else {
      in0 += (int64_t)i * d.in_is;
      out0 += (int64_t)i * d.out_is;
    }
    [[maybe_unused]] const unsigned row_ub = o * inner + i;     // UNEVEN: row of the exchange buffer
    // (... whose blocks are all at least a thread group wide: the group form of the block look-up, fft_pow2_impl.h; uniform)
    [[maybe_unused]] const bool ub_group = UNEVEN && d.ub_minw >= (NTL > NTS ? NTL : NTS);
    cx<real> v[R];
    // Split layouts: thread slots e = t + q*NT advance by NT, and a block of the cut axis holds
    // (R >> lgp) * NT entries, so block boundaries fall between the same q for every thread: a
    // workgroup-uniform counter adds the block jump to the (uniform) step -- scalar work only.
    const int seg_in = RL >> L_in_lgp, seg_out = RS >> L_out_lgp;
    if constexpr (NTL < NT) valid = valid && t < NTL;               // (thread rows beyond the load / store geometry)
    if constexpr (NTS < NT) valid_st = valid_st && t < NTS;
    if constexpr (ORDER) {
      // (every slot index a constant: one unrolled copy of the loop per rotation, picked by a uniform branch)
      if (valid) {
        const int64_t idx0 = in0 + (int64_t)tl * d.in_es;
        auto issue = [&](auto q0c) {
          constexpr int Q0 = decltype(q0c)::value;
#pragma unroll
          for (int i = 0; i < RL; ++i) {
            const int q = (i + Q0) % RL;
            v[q] = tile_load<real, IOMODE, NT_LD>(d, in, in0, idx0 + (int64_t)q * q_in, tl + q * NTL, sy_in);
          }
        };
        switch (ord_q0) {
          default: issue(std::integral_constant<int, 0>()); break;
          case 1: issue(std::integral_constant<int, RL / 4>()); break;
          case 2: issue(std::integral_constant<int, RL / 2>()); break;
          case 3: issue(std::integral_constant<int, 3 * RL / 4>()); break;
        }
      } else {
#pragma unroll
        for (int q = 0; q < R; ++q) v[q] = {0, 0};
      }
    } else if (valid) {
      int64_t idx = in0 + t_in;
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < RL; ++q) {
        if constexpr (TRUNC) {
          if constexpr (HALF && TRUNC_LOAD) {
            // zero-padded half spectrum (libfft.py:298-311): entries >= tr_n are zero, the last kept
            // entry of an even truncated length is a real Nyquist value taken at half weight
            const int e = tl + q * NTL;
            const bool ok = e < d.tr_n, nyq = d.tr_even && e == d.tr_n - 1;
            if constexpr (UNEVEN) v[q] = reinterpret_cast<const cx<real> *>(in)[uneven_offset(d, row_ub, o, i, ok ? e : 0)];
            else v[q] = reinterpret_cast<const cx<real> *>(in)[ok ? idx : in0];
            v[q].x *= ok ? (nyq ? (real)0.5 : (real)1) : (real)0;
            v[q].y *= (ok && !nyq) ? (real)1 : (real)0;
          } else if constexpr (TRUNC_LOAD) v[q] = tile_load_pad<real, IOMODE>(d, in, in0, idx, pad_shift_in, tl + q * NTL, sy_in);
          else v[q] = tile_load<real, IOMODE, false>(d, in, in0, idx, tl + q * NTL, DEFER_SIGN ? (real)1 : sy_in);
        } else if constexpr (MODE == MODE_C2R_H && UNEVEN) {
          v[q] = reinterpret_cast<const cx<real> *>(in)[ub_group ? uneven_offset_group<NTL>(d, row_ub, o, i, tl, q) : uneven_offset(d, row_ub, o, i, tl + q * NTL)];
        } else if constexpr (SYS_LD) {
          v[q] = sys_in.template ld<real>(idx);
          // (packed-real rows never conjugate on load -- conj_in = 0, half_desc / plan_fused3 rows -- and with the sign applied
          // here the compiler waited for every load of the c2r rows before it issued the next: 16 round trips to the ring per tile)
          if constexpr (!HALF) v[q].y *= sy_in;
        } else {
          // (unequal-width stage kernels: the sign of the imaginary parts goes on behind ALL the loads, below -- applied to
          // each value as it arrives, under their register pressure, the compiler waited for every load before issuing the next)
          v[q] = tile_load<real, IOMODE, NT_LD>(d, in, in0, idx, tl + q * NTL, DEFER_SIGN ? (real)1 : sy_in);
        }
        int64_t step = q_in;
        if (++cnt == seg_in) {
          cnt = 0;
          step += L_in_jump;
        }
        idx += step;
      }
    } else {
#pragma unroll
      for (int q = 0; q < R; ++q) v[q] = {0, 0};
    }
    if constexpr (DEFER_SIGN && !NO_SIGN) {
      if (d.conj_in) {
#pragma unroll
        for (int q = 0; q < RL; ++q) v[q].y = -v[q].y;
      }
    }
    GFFT_AFTER_LOADS
    // Launder the (loop-invariant) twiddle table pointer once per tile: otherwise LICM hoists every
    // stage's twiddle loads out of the tile loop and parks them in VGPRs for the whole kernel
    // (40 VGPRs at fp64 n=1024), costing a wave of occupancy per SIMD.
    const cx<real> *twl = tw;
    asm volatile("" : "+s"(twl));
    [[maybe_unused]] const cx<real> *rtw = reinterpret_cast<const cx<real> *>(d.rtw);
    if constexpr (HALF) asm volatile("" : "+s"(rtw));
    if constexpr (MODE == MODE_C2R_H) {
      // Hermitian half spectrum X[0..N] -> packed spectrum Z[0..N-1], conjugated for the
      // inverse-by-conjugation butterflies.  Imaginary parts of X[0] and X[N] are ignored, as FFTW's
      // c2r does.
      cx<real> top = {0, 0};
      if (tl == 0) {
        if constexpr (UNEVEN && !TRUNC) {
          if (valid) top.x = reinterpret_cast<const cx<real> *>(in)[uneven_offset(d, row_ub, o, i, N)].x;
        } else if constexpr (SYS_LD) {
          if (valid) top.x = sys_in.template ld<real>(in0 + (int64_t)N * d.in_es).x;
        } else if constexpr (!TRUNC_LOAD) {
          if (valid) top.x = reinterpret_cast<const cx<real> *>(in)[in0 + (int64_t)N * d.in_es].x;
        }
        v[0].y = 0;
      }
      const cx<real> wt = rtw[(NTL < NT && tl >= NTL) ? 0 : tl];
      mirror_pass<real, N, RL, SPLIT, WL, PADSH>(v, tl, col, top, [&](int q, cx<real> p) {
        const cx<real> w = mirror_twiddle<real, RL>(wt, q);        // (c, s) = exp(-2 pi i e / 2N)
        const cx<real> a = {v[q].x + p.x, v[q].y - p.y};           // X + conj P
        const cx<real> b = {v[q].x - p.x, v[q].y + p.y};           // X - conj P
        const cx<real> wb = {w.x * b.x + w.y * b.y, w.x * b.y - w.y * b.x};   // conj(w) b
        v[q] = {a.x - wb.y, -(a.y + wb.x)};                        // conj(a + i conj(w) b)
      }, NTL == NT || tl < NTL);
      // Pin the line here: left free, the scheduler interleaves this pass with the first butterfly
      // stage and keeps both generations of the line alive (fp32 R = 16: 175 VGPRs -> 107).
#pragma unroll
      for (int q = 0; q < RL; ++q) asm volatile("" : "+v"(v[q].x), "+v"(v[q].y));
    }
    // (the row index `tl` is laundered for the same reason: fp32 n=1024 R=32 104 bytes of scratch
    // -> none; fp64 n=1024 R=16 T=16 127 -> 107 VGPRs)
    if constexpr (!ACCESS_ONLY) {
      if constexpr (GEO::UNIFORM) Stage<real, N, R, SPLIT, WL, PADSH, 1, RADS...>::run(v, tl, col, twl);
      else StageV<real, N, R, SPLIT, 1, RADS...>::run(v, tl, col, twl);
    }
    if constexpr (!HALF && !NO_PIN) {
      // pin the line between the last stage and the stores: interleaved by the scheduler the two
      // keep extra copies alive (fp32 n = 1024 R = 32 with the truncating store: 145 spilled VGPRs
      // -> 11; the plain fp32 R = 32 pass: 127 VGPRs + 4 spilled -> 121, none)
#pragma unroll
      for (int q = 0; q < RS; ++q) asm volatile("" : "+v"(v[q].x), "+v"(v[q].y));
    }
    GFFT_PHASE(5)
    [[maybe_unused]] cx<real> z0 = v[0];
    if constexpr (MODE == MODE_R2C_H) {
      // packed spectrum Z[0..N-1] -> Hermitian half spectrum X[0..N-1] in place (twice the values:
      // the factor 1/2 rides on the store scale); X[N] = Re Z[0] - Im Z[0] is stored by thread 0
      const cx<real> wt = rtw[(NTS < NT && tl >= NTS) ? 0 : tl];
      mirror_pass<real, N, RS, SPLIT, WL, PADSH>(v, tl, col, v[0], [&](int q, cx<real> p) {
        const cx<real> w = mirror_twiddle<real, RS>(wt, q);
        const cx<real> a = {v[q].x + p.x, v[q].y - p.y};           // Z + conj P
        const cx<real> b = {v[q].x - p.x, v[q].y + p.y};           // Z - conj P
        const cx<real> wb = cmul(w, b);
        v[q] = {a.x + wb.y, a.y - wb.x};                           // a - i w b
      }, NTS == NT || tl < NTS);
    }
    if constexpr (TRUNC && !TRUNC_LOAD && MODE == MODE_C2C && !HALF) {
      // complex truncation with even N: entries h = N/2 and n - h of the padded spectrum both land
      // on truncated entry h (libfft.py:281-284).  They live in different threads: pass the upper
      // one through LDS.  (uniform branch: every thread of the workgroup takes it or none does)
      if (d.tr_even) {
        cx<real> *fold = reinterpret_cast<cx<real> *>(smem);
        const int h = d.tr_N >> 1;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RS; ++q)
          if ((NTS == NT || tl < NTS) && tl + q * NTS == d.n - h) fold[c] = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RS; ++q)
          if ((NTS == NT || tl < NTS) && tl + q * NTS == h) v[q] = v[q] + fold[c];
        // (barrier-free exchanges: a wave running ahead must not start the next tile's exchange -- the first
        // row's region holds `fold` -- before every wave has read it)
        if constexpr (WL) __syncthreads();
      }
    }
    if constexpr (BIGTW && (TRANSPOSE || SYS_ST)) {
      // four-step twiddle W^(m e), e = t + q NT: two table look-ups per THREAD -- W^(m t) and
      // W^(m NT) -- and the powers of the second by squaring (q is a compile-time index, so entry q
      // costs at most log2 R multiplications); one look-up pair per ELEMENT tripled the load
      // instructions of this pass (data + 2 gathers)
      const auto big = [&](unsigned x) {
        const cx<real> a = reinterpret_cast<const cx<real> *>(d.tw_hi)[x >> d.tw_L];
        const cx<real> b = reinterpret_cast<const cx<real> *>(d.tw_lo)[x & ((1u << d.tw_L) - 1)];
        return cmul(a, b);
      };
      constexpr int LG = R >= 32 ? 5 : (R >= 16 ? 4 : (R >= 8 ? 3 : 2));
      static_assert((1 << LG) >= R, "powers of the step twiddle");
      const cx<real> w0 = big(m * (unsigned)tl);
      cx<real> sp[LG];
      sp[0] = big(m * (unsigned)NT);
#pragma unroll
      for (int k = 1; k < LG; ++k) sp[k] = cmul(sp[k - 1], sp[k - 1]);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        cx<real> w = w0;
#pragma unroll
        for (int k = 0; k < LG; ++k)
          if ((q >> k) & 1) w = cmul(w, sp[k]);
        v[q] = cmul(v[q], w);
      }
    }
    if constexpr (TRANSPOSE) {
      // Transposing store.  Loads ran with lanes along T adjacent columns (T*16-byte segments of the
      // strided input); the output of each column is one contiguous line, so storing in the same
      // mapping would write T short runs per instruction.  Finish the element-wise work here
      // (four-step twiddle, scale), transpose the thread grid through LDS -- thread (c, t) hands
      // its R values to thread (c' = tid / NT, t' = tid % NT), same slots e = t' + q*NT -- and
      // store with lanes along e: whole 64-lane rows of one output line.
      // The mirror image, a ROW pass (!COLS: the second four-step pass on an intermediate it can read as rows):
      // lanes ran along e of ONE row; its output entries lie out_es apart but those of T adjacent rows side by
      // side, so the grid is transposed the other way and the stores run with lanes along the T rows.
      static_assert(SPLIT && MODE == MODE_C2C && (COLS ? BIGTW : !BIGTW), "transposing store: a four-step pass");
#pragma unroll
      for (int q = 0; q < R; ++q) {
        v[q].x *= sx_out;
        v[q].y *= sy_out;
      }
      constexpr int PAD = PADSH;
      const int c2 = COLS ? tid / NT : tid % T, t2 = COLS ? tid % NT : tid / T;
      real *w = reinterpret_cast<real *>(col);
      real *r = reinterpret_cast<real *>(smem + (size_t)c2 * CS * WORD);
      const int wb = pad_slot<PAD>(t), rb = pad_slot<PAD>(t2);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < R; ++q) w[wb + pad_slot<PAD>(q * NT)] = v[q].x;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < R; ++q) v[q].x = r[rb + pad_slot<PAD>(q * NT)];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < R; ++q) w[wb + pad_slot<PAD>(q * NT)] = v[q].y;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < R; ++q) v[q].y = r[rb + pad_slot<PAD>(q * NT)];
      // the column this thread now stores (flat tiling, as the BIGTW passes use)
      const unsigned b2 = tile * T + c2;
      if (b2 < batch) {
        const unsigned bm2 = b2 / inner, i2 = b2 - bm2 * inner, o2 = bm2 / mid, m2 = bm2 - o2 * mid;
        int64_t idx = (int64_t)o2 * d.out_os + (int64_t)m2 * d.out_ms + (int64_t)i2 * d.out_is +
                      (int64_t)t2 * d.out_es;
#pragma unroll
        for (int q = 0; q < R; ++q) {
          if constexpr (SYS_ST) sys_out.template st<real>(idx, v[q]);
          else stc<real, NT_ST>(reinterpret_cast<cx<real> *>(out) + idx, v[q]);
          idx += q_out;
        }
      }
      // (barrier-free exchanges: a wave running ahead must not start the next tile's exchange in a region the
      // others are still reading)
      if constexpr (WL) __syncthreads();
    } else if constexpr (ORDER) {
      if (valid_st) {
        const int64_t idx0 = out0 + (int64_t)tl * d.out_es;
        auto issue = [&](auto q0c) {
          constexpr int Q0 = decltype(q0c)::value;
#pragma unroll
          for (int i = 0; i < RS; ++i) {
            const int q = (i + Q0) % RS;
            tile_store<real, IOMODE, false, NT_ST>(d, out, idx0 + (int64_t)q * q_out, tl + q * NTS, m, v[q], sx_out, sy_out);
          }
        };
        switch (ord_q0) {
          default: issue(std::integral_constant<int, 0>()); break;
          case 1: issue(std::integral_constant<int, RS / 4>()); break;
          case 2: issue(std::integral_constant<int, RS / 2>()); break;
          case 3: issue(std::integral_constant<int, 3 * RS / 4>()); break;
        }
      }
    } else if (valid_st) {
      int64_t idx = out0 + t_out;
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < RS; ++q) {
        if constexpr (TRUNC) {
          if constexpr (HALF && !TRUNC_LOAD) {
            // truncated half spectrum (libfft.py:286-296): keep entries < tr_n; the last one of an
            // even truncated length becomes a real Nyquist value of twice the weight
            const int e = tl + q * NTS;
            if (e < d.tr_n) {
              const bool nyq = d.tr_even && e == d.tr_n - 1;
              int64_t at = idx;
              if constexpr (UNEVEN) at = uneven_offset(d, row_ub, o, i, e);
              reinterpret_cast<cx<real> *>(out)[at] = {v[q].x * (nyq ? 2 * sx_out : sx_out), nyq ? (real)0 : v[q].y * sy_out};
            }
          } else if constexpr (!TRUNC_LOAD) tile_store_trunc<real, IOMODE>(d, out, idx, pad_shift_out, tl + q * NTS, v[q], sx_out, sy_out);
          else tile_store<real, IOMODE, false, false>(d, out, idx, tl + q * NTS, m, v[q], sx_out, sy_out);
        } else if constexpr (MODE == MODE_R2C_H && UNEVEN) {
          reinterpret_cast<cx<real> *>(out)[ub_group ? uneven_offset_group<NTS>(d, row_ub, o, i, tl, q) : uneven_offset(d, row_ub, o, i, tl + q * NTS)] = {v[q].x * sx_out, v[q].y * sy_out};
        } else if constexpr (SYS_ST) {
          sys_out.template st<real>(idx, cx<real>{v[q].x * sx_out, v[q].y * sy_out});
        } else {
          tile_store<real, IOMODE, BIGTW, NT_ST>(d, out, idx, tl + q * NTS, m, v[q], sx_out, sy_out);
        }
        int64_t step = q_out;
        if (++cnt == seg_out) {
          cnt = 0;
          step += L_out_jump;
        }
        idx += step;
      }
      if constexpr (MODE == MODE_R2C_H && UNEVEN && !TRUNC) {
        if (tl == 0)
          reinterpret_cast<cx<real> *>(out)[uneven_offset(d, row_ub, o, i, N)] = {(z0.x - z0.y) * 2 * sx_out, 0};
      } else if constexpr (MODE == MODE_R2C_H && !TRUNC) {
        // X[N] from thread 0, followed by L_out_pad zeros from its neighbours: one coalesced store
        // that completes the row's last 128-byte line when the output rows are pitched
        if (tl <= L_out_pad) {
          const cx<real> last = {tl == 0 ? (z0.x - z0.y) * 2 * sx_out : (real)0, 0};
          if constexpr (SYS_ST) sys_out.template st<real>(out0 + (int64_t)(N + tl) * d.out_es, last);
          else reinterpret_cast<cx<real> *>(out)[out0 + (int64_t)(N + tl) * d.out_es] = last;
        }
      }
    }
  }
