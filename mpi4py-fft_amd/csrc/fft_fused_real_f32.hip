// fp32 fused pass pairs of REAL 3-D transforms (the fp64 ones: fft_fused_real_f64.hip; the kernel: fft_pow2_impl.h
// fft_fused2_kernel): [packed-real r2c rows of 1024 reals -> strided n = 1024] on the contiguous planes i0 of the r2c
// schedule, [strided n = 1024 -> packed-real c2r rows] on the planes i1 of the c2r schedule -- 1024^3 real fp32, the
// single-GPU relative of BASELINE config C5.  1024-thread workgroups: rows 16 values per thread (c2r: 8, the R = 16
// c2r plan needs ~170 VGPRs), strided 32 values per thread on 32 columns (256-byte segments).
// FUSED_R2C_PLANES_B / FUSED_COLS_C2R_B: the same pairs as the two local stages of a real slab-decomposed transform
// (gfft_plan_create_guru2_real), the strided side in equal blocks of the all-to-all buffer (PF_BLOCKS_OUT / PF_BLOCKS_IN).
#include "fft_fused_impl.h"

namespace gfft {

//                           real   N    R   T  COLS   SPLIT  FLAGS                 MODE        BIGTW  radices
typedef PassCfg<float, 512, 16, 32, false, false, PF_NT_LOAD | PF_SYS_STORE | PF_NATURAL, MODE_R2C_H, false, 16, 8, 4> R2CRows512ToRingF32;
typedef PassCfg<float, 512, 8, 16, false, false, PF_NT_STORE | PF_SYS_LOAD | PF_NATURAL, MODE_C2R_H, false, 8, 8, 8> C2RRows512FromRingF32;
typedef PassCfg<float, 1024, 32, 32, true, true, PF_NT_LOAD | PF_C2C_ONLY | PF_SYS_STORE | PF_NATURAL, MODE_C2C, false, 16, 16, 4> Cols1024ToRingF32;
typedef PassCfg<float, 1024, 32, 32, true, true, PF_NT_STORE | PF_C2C_ONLY | PF_SYS_LOAD | PF_NATURAL, MODE_C2C, false, 16, 16, 4> Cols1024FromRingF32;
typedef PassCfg<float, 1024, 32, 32, true, true, PF_NT_LOAD | PF_C2C_ONLY | PF_SYS_STORE | PF_NATURAL | PF_BLOCKS_IN, MODE_C2C, false, 16, 16, 4> Cols1024ToRingBF32;
typedef PassCfg<float, 1024, 32, 32, true, true, PF_NT_STORE | PF_C2C_ONLY | PF_SYS_LOAD | PF_NATURAL | PF_BLOCKS_OUT, MODE_C2C, false, 16, 16, 4> Cols1024FromRingBF32;

const FusedPair *fused2_select_real_f32(int kind, int n_a, int n_b) {
  const bool r2c = kind == FUSED_R2C_PLANES || kind == FUSED_R2C_PLANES_B;
  if (r2c ? !(n_a == 512 && n_b == 1024) : !(n_a == 1024 && n_b == 512)) return nullptr;
  switch (kind) {
    case FUSED_R2C_PLANES: return fused_pair<R2CRows512ToRingF32, Cols1024FromRingF32>();
    case FUSED_COLS_C2R: return fused_pair<Cols1024ToRingF32, C2RRows512FromRingF32>();
    case FUSED_R2C_PLANES_B: return fused_pair<R2CRows512ToRingF32, Cols1024FromRingBF32>();
    case FUSED_COLS_C2R_B: return fused_pair<Cols1024ToRingBF32, C2RRows512FromRingF32>();
  }
  return nullptr;
}

}  // namespace gfft
