// fp64 fused pass pairs of REAL 3-D transforms (fft_pow2_impl.h fft_fused2_kernel; the complex pairs: fft_fused_f64.hip):
//   FUSED_R2C_PLANES  [packed-real r2c rows of 2 N reals -> strided n]   passes 1 + 2 of the r2c schedule, plane = one i0:
//                     its n1 rows are contiguous in the caller's array, the half spectrum (N + 1 entries, the row's last
//                     line completed with zeros) goes into the slot, the strided pass takes it along axis 1
//   FUSED_COLS_C2R    [strided n -> packed-real c2r rows]                passes 2 + 3 of the c2r schedule, plane = one i1
//   FUSED_R2C_PLANES_B / FUSED_COLS_C2R_B   the same pairs as the two LOCAL stages of a real slab-decomposed transform
//                     (gfft_plan_create_guru2_real): the strided side is the all-to-all buffer, its axis cut into equal blocks
//                     (PF_BLOCKS_OUT / PF_BLOCKS_IN, fft_pow2_body.inc), rows exactly N + 1 entries apart there
// The reference's default dtype is `float` (mpifft.py:202), i.e. these are the transforms a PFFT runs unless told otherwise
// (libfft.py:48-79, fftw/xfftn.py:173-326: the Hermitian axis is the last one, N / 2 + 1 entries).
// Rows: 16 values per thread, a row inside one wave (exchanges without barriers); strided: 32 values per thread, one
// exchange; 512 threads both, one workgroup per CU.
#include "fft_fused_impl.h"
#include <cstdlib>

namespace gfft {

// option c2r_2048: the c2r pair on rows of 2048 reals.  Round 4 measured it losing -- (1024,1024,2048) backward 21.4 -> 28.1 ms,
// every memory phase of its tiles 2-3 x slower than at 1024 reals -- and left it off, unexplained.  Round 5: the workspace
// pitch of that shape was 1032 = 8 x 129 entries, the one multiplier the channel hash folds onto itself (plan.cpp
// plan_fused3, pitch129); on 1040 entries the pair runs 11.8 ms against 5.8 + 6.7 for its two passes, the step 37.85 ->
// 36.33 ms (profiles/r05_ab_pitch129.txt).
int g_c2r_2048 = 1;

//                            real    N    R   T  COLS   SPLIT FLAGS                 MODE        BIGTW  radices
typedef PassCfg<double, 512, 16, 16, false, true, PF_NT_LOAD | PF_SYS_STORE | PF_NATURAL, MODE_R2C_H, false, 16, 8, 4> R2CRows512ToRing;      // 1024 reals per row
typedef PassCfg<double, 1024, 16, 8, false, true, PF_NT_LOAD | PF_SYS_STORE | PF_NATURAL, MODE_R2C_H, false, 16, 16, 4> R2CRows1024ToRing;    // 2048 reals per row
typedef PassCfg<double, 512, 16, 16, false, true, PF_NT_STORE | PF_SYS_LOAD | PF_NATURAL, MODE_C2R_H, false, 16, 8, 4> C2RRows512FromRing;
typedef PassCfg<double, 1024, 16, 8, false, true, PF_NT_STORE | PF_SYS_LOAD | PF_NATURAL, MODE_C2R_H, false, 16, 16, 4> C2RRows1024FromRing;     // 2048 reals per row (option c2r_2048)
typedef PassCfg<double, 1024, 32, 16, true, true, PF_NT_LOAD | PF_C2C_ONLY | PF_SYS_STORE | PF_NATURAL, MODE_C2C, false, 32, 32> Cols1024ToRing;
typedef PassCfg<double, 1024, 32, 16, true, true, PF_NT_STORE | PF_C2C_ONLY | PF_SYS_LOAD | PF_NATURAL, MODE_C2C, false, 32, 32> Cols1024FromRing;
// the strided side of the slab pairs: the array side in equal blocks of the strided axis (the complex pairs' ColsToRingB / ColsFromRingB)
typedef PassCfg<double, 1024, 32, 16, true, true, PF_NT_LOAD | PF_C2C_ONLY | PF_SYS_STORE | PF_NATURAL | PF_BLOCKS_IN, MODE_C2C, false, 32, 32> Cols1024ToRingB;
typedef PassCfg<double, 1024, 32, 16, true, true, PF_NT_STORE | PF_C2C_ONLY | PF_SYS_LOAD | PF_NATURAL | PF_BLOCKS_OUT, MODE_C2C, false, 32, 32> Cols1024FromRingB;

const FusedPair *fused2_select_real_f64(int kind, int n_a, int n_b) {
  const bool r2c = kind == FUSED_R2C_PLANES || kind == FUSED_R2C_PLANES_B, c2r = kind == FUSED_COLS_C2R || kind == FUSED_COLS_C2R_B;
  if (r2c && !((n_a == 512 || n_a == 1024) && n_b == 1024)) return nullptr;
  if (c2r && !(n_a == 1024 && (n_b == 512 || (n_b == 1024 && g_c2r_2048 != 0)))) return nullptr;
  switch (kind) {
    case FUSED_R2C_PLANES: return n_a == 512 ? fused_pair<R2CRows512ToRing, Cols1024FromRing>() : fused_pair<R2CRows1024ToRing, Cols1024FromRing>();
    case FUSED_COLS_C2R: return n_b == 1024 ? fused_pair<Cols1024ToRing, C2RRows1024FromRing>() : fused_pair<Cols1024ToRing, C2RRows512FromRing>();
    case FUSED_R2C_PLANES_B: return n_a == 512 ? fused_pair<R2CRows512ToRing, Cols1024FromRingB>() : fused_pair<R2CRows1024ToRing, Cols1024FromRingB>();
    case FUSED_COLS_C2R_B: return n_b == 1024 ? fused_pair<Cols1024ToRingB, C2RRows1024FromRing>() : fused_pair<Cols1024ToRingB, C2RRows512FromRing>();
  }
  return nullptr;
}

}  // namespace gfft
