// Fused pass pairs: what the four tables fft_fused_f64.hip / _f32.hip / _real_f64.hip / _real_f32.hip share.  A pair exists for a
// (precision, n) when both passes -- the row plan and the strided plan of the stand-alone tables
// (fft_pow2_f64.hip / fft_pow2_f32.hip), rebuilt on 1024-thread workgroups -- fit one workgroup shape.
#pragma once
#include "fft_pow2_impl.h"

namespace gfft {

// (FLAGS of the hand-off sides: PF_SYS_STORE / PF_SYS_LOAD on PF_NATURAL layouts; PF_C2C_ONLY = plain complex strided pass,
// PF_TRANSPOSE_STORE = first four-step pass -- gfft_internal.h)
template <typename real, int N> struct FusedCfgs;

// the FusedPair of two PassCfgs: tile counts and launch of the SAME two configurations
template <typename A, typename B>
const FusedPair *fused_pair() {
  static const FusedPair p = {&A::ntiles, &B::ntiles, &launch_fused2<A, B>};
  return &p;
}

// the complex kinds on one set of configurations C (tiles per plane of either pass: rows and four-step first passes tile the
// flat batch, strided passes the columns of each row of the batch)
template <typename C>
static const FusedPair *pair_of_kind(int kind) {
  switch (kind) {
    case FUSED_PLANES_2D:
    case FUSED_ROWS_COLS: return fused_pair<typename C::RowsToRing, typename C::ColsFromRing>();
    case FUSED_COLS_ROWS: return fused_pair<typename C::ColsToRing, typename C::RowsFromRing>();
    case FUSED_FOURSTEP: return fused_pair<typename C::FourStepFirst, typename C::ColsFromRing>();
    case FUSED_FOURSTEP_ROWS: return fused_pair<typename C::FourStepFirstNat, typename C::RowsFromRingT>();
  }
  return nullptr;
}

// the tables of the other three files, behind fused2_select (fft_fused_f64.hip)
const FusedPair *fused2_select_f32(int kind, int n_a, int n_b);
const FusedPair *fused2_select_real_f64(int kind, int n_a, int n_b);
const FusedPair *fused2_select_real_f32(int kind, int n_a, int n_b);

}  // namespace gfft
