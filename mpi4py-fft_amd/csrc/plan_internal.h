// What the planner (plan.cpp) and the C surface (api.cpp) share: the plan and what it is made of, and the planner functions the
// entry points call.  For those two files only -- kernel files include gfft_internal.h and never see a plan.
#pragma once
#include "../../include/gfft.h"
#include "gfft_internal.h"

#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

namespace gfft {

// ---- tunables ---------------------------------------------------------------------------
struct Options {
  int grid_cap = 0;          // workgroups per launch at most; 0 = 4096, and 16384 for the passes of complex 3-D schedules
  int variant_rows = 0;
  int variant_cols = 0;
  int force_generic = 0;
  int xcd_swizzle = -1;      // XCD-contiguous tile order in the pow2 kernels: 0 off, 1 on, -1 auto
  int tile_order = -1;       // order in time of tiles and rows inside an XCD-contiguous walk (PassDesc::order): -1 = each plan's own, >= 0: this one (0 = plain); read at launch time (A/B on one plan)
  int profile = 0;           // record HIP events around every pass (bench.py roofline leg)
  int fused3 = 1;            // reorder + padded-pitch workspace for 3-D all-axes plans
  int debug_flat = 0;        // gfft_debug_pass: tiles over the flattened (mid, inner) index
  int flat_out = 1;          // forward r2c 3-D plans: far-axis last pass with flattened tiles
  int mixv_variant = 0;      // A/B: alternative kernels of the unequal-width lengths (tools/gen_mixv_tables.py)
  int mixv = 1;              // one-pass kernels for 3 x 5 x 2^k lengths (fft_mixv_*.hip); 0: the two-pass plans of rounds 1-4 (A/B)
  int wtile = 1;             // tile-major workspace under the complex 3-D pair schedule (plan_fused3; A/B)
  int plane2d = 1;           // planes of 32^2 / 64^2 points: both passes in one launch, the plane in LDS (fft_plane2d.hip; 0: two passes, A/B)
  int fuse2 = 1;             // pass pairs in one persistent launch, handed over through the Infinity Cache (fft_fused_f64.hip)
  int fuse2_ring = 0, fuse2_lag = 0;   // slots of the hand-off ring / planes the producer runs ahead; 0 = auto (fused2_ring)
  int fuse2_kinds = 2046;    // which pairs (bit = FusedKind): measured per kind, see fused2_pair (bits 1-10; 0, [rows -> strided] of the 3-D schedule, off)
  int fuse2_f32 = 1;         // 1: complex64 pairs (fft_fused_f32.hip); 2: the real fp32 pairs too (fft_fused_real_f32.hip: measured level, off)
  int fuse2_wait_ms = 2000;  // wall-clock limit of one wait inside a fused launch before the launch is voided (0: at once -- test hook)
  int debug_tile_lg = 0, debug_tile_side = 0, debug_tile_stride = 0;   // gfft_debug_pass: tile-major lines (rows passes)
  int64_t fused3_min_bytes = 32 << 20;
  // TEST HOOK (tests/test_gpu_rounding_guard.py): twiddle tables uploaded while debug_tw_exp > 0 carry ONE wrong entry --
  // the real part of entry debug_tw_index (mod n) is off by 10^-debug_tw_exp -- under their own cache key, so that plans made
  // before / after are untouched.  What the rounding-level guards of the test suite must catch; never set by the product.
  // debug_tw_len != 0: only the table of exactly that length (a packed-real plan's rtw(n), say, and not its tw(n/2)).
  int debug_tw_index = 1, debug_tw_exp = 0, debug_tw_len = 0;
  // TEST HOOK (tests/test_gpu_r2r_guard.py): the same for the pre / post tables of the real-to-real kinds (get_r2r_tables) --
  // tables uploaded while debug_r2r_exp > 0 carry ONE wrong entry: the real part of entry debug_r2r_index (mod n) of `pre`
  // (debug_r2r_post = 0) or `post` (1) is off by 10^-debug_r2r_exp -- under their own cache key, so that plans made
  // before / after are untouched.  What the rounding-level guards of the test suite must catch; never set by the product.
  int debug_r2r_index = 1, debug_r2r_exp = 0, debug_r2r_post = 0;
  Options();                 // reads the environment variables of the option table (api.cpp kOptions)
};

struct BigTw { void *hi, *lo; int L; };         // the two-level twiddle table of a four-step length (get_bigtw)
struct R2RTables { void *pre, *post; };         // the pointwise tables of a real-to-real kind (get_r2r_tables)

// ---- plan -------------------------------------------------------------------------------
// Buffers a pass may read/write.  IN/OUT are the caller's arrays; the other three are regions of
// one plan-owned scratch allocation (made at the first execute):
//   WS   an array-sized workspace: the padded-pitch W of the 3-D schedule, or the complex staging
//        of a multi-axis c2r (so the caller's input is never written)
//   FS   the transposed intermediate of a four-step axis
//   AUX  the embedding buffer of a Bluestein / real-as-complex axis
//   RING the hand-off ring (+ its counters) of a fused pass pair (PK_FUSED2)
//   FS2  the intermediate of the outer level of a three-pass axis (lengths beyond 2^24, plan_long)
enum Buf { BUF_IN = 0, BUF_OUT = 1, BUF_WS = 2, BUF_FS = 3, BUF_AUX = 4, BUF_RING = 5, BUF_FS2 = 6, BUF_COUNT = 7 };

enum PassKind { PK_FFT = 0, PK_EMBED, PK_MULB, PK_EXTRACT, PK_FUSED2, PK_PLANE2D };    // PK_PLANE2D: both passes of small planes on chip (fft_plane2d.hip)

struct Pass {
  PassKind kind = PK_FFT;
  PassDesc d{};
  Factors f{};
  bool regk = false, cols = false;   // register-resident kernel family (else fft_generic); mapping
  int src = BUF_IN, dst = BUF_OUT;
  bool carries_scale = false;        // the plan's scale factor is applied by this pass
  bool logical_first = false;        // first kernel of a transformed axis (profiling/report)
  PointDesc pt{};                    // PK_EMBED / PK_MULB / PK_EXTRACT geometry
  double extra_scale = 1.0;          // e.g. 1/M of Bluestein's inverse
  // packed-real passes keep the full-length form of the same line (MODE_R2C / MODE_C2R with the
  // zero-imaginary / mirror adapters) for what only that form can fuse: truncation / padding
  bool has_full = false;
  PassDesc full{};
  int64_t data_inner = 0;            // columns of d.inner that carry data (0 = all): byte accounting
  // guru plans: blocks of the transformed axis per side and the distance between their starts
  // (gfft_plan_set_tiles re-derives the block jumps from them)
  int blocks[2] = {1, 1};
  int64_t bstride[2] = {0, 0};
  // PK_FUSED2: `d` = pass A on ONE plane, `d2` = pass B on one plane, `fused` = the planes (fft_pow2_impl.h
  // fft_fused2_kernel); fused.ctr and the ring's address are filled in at execution
  PassDesc d2{};
  FusedDesc fused{};
  int fused_kind = 0;
  const FusedPair *pair = nullptr;   // the kernel pair, resolved when the plan was made (fused2_pair)
  PassDesc *dev_descs = nullptr;     // {d, d2} in device memory (owned by the plan: gfft_plan_s::device_allocs)
  // the same two passes as stand-alone launches (gfft_plan_s::alt[alt_first], [alt_first + 1]): what the plan runs
  // once a fused launch has given up a wait; alt_buf / alt_bytes = the scratch region only that form needs
  int alt_first = -1;
  int alt_buf = -1;
  size_t alt_bytes = 0;
  double bytes2 = 0;                 // algorithmic bytes of pass B (gfft_plan_pass_info reports A + B)
  mutable LaunchNote launched{};     // TEST AID (gfft_plan_pass_launch): tiles / workgroups of this pass's most recent launch
};

struct PairChoice {                 // what fused2_pair answers
  const FusedPair *pair = nullptr;
  int ring = 0, lag = 0;
};

// A batch of 1-D lines: array [outer][nin -> nout][inner] (row-major), logical length n.
struct Line {
  int64_t outer, inner, n, nin, nout;
  int mode;        // PassMode
  bool inverse;
  int src, dst;
};

// ---- scratch shared by all plans ---------------------------------------------------------------
// One buffer per (device, host thread, stream) -- torch's default stream is handle 0 on EVERY device --, grown to the
// largest request seen there: the passes of one
// gfft_execute are enqueued back to back by one thread and a stream runs them in order, so every
// plan that thread executes on that stream can share the buffer (the forward and the backward plan
// of a 1024^3 PFFT each need a 16 GiB padded workspace; owning one each doubled that).  Other
// threads -- whose launches could interleave with this one's on the same stream -- and other
// streams get their own.  Growing synchronises the stream once (earlier launches may still be
// using the old buffer).
struct ScratchPool {
  struct Slot { void *p = nullptr; size_t n = 0; bool pinned = false; };
  struct Key {
    int dev; std::thread::id th; hipStream_t st;
    bool operator<(const Key &o) const { return std::tie(dev, th, st) < std::tie(o.dev, o.th, o.st); }
  };
  std::mutex m;
  std::map<Key, Slot> bufs;
  std::vector<void *> retired;      // buffers a captured graph may still use, replaced by larger ones
  int get(hipStream_t s, size_t bytes, void **out) {
    std::lock_guard<std::mutex> lock(m);
    const auto me = std::this_thread::get_id();
    const int dev = current_device();
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone) {
      // No allocation inside a capture: the graph uses the buffer this thread's warm-up execution
      // grew (on whatever stream that ran), so replays must not overlap other executions of this
      // thread -- the stream a graph is replayed on orders them.  The buffer's address is now baked
      // into the graph: it is PINNED -- never freed by growth or by the last plan going away, only
      // by an explicit gfft_scratch_release().
      for (auto &kv : bufs)
        if (kv.first.dev == dev && kv.first.th == me && kv.second.n >= bytes) { kv.second.pinned = true; *out = kv.second.p; return GFFT_OK; }
      return fail(GFFT_ERR_INVALID, "stream capture: execute the plan once before capturing it (its workspace is allocated at the first execution)");
    }
    Slot &b = bufs[Key{dev, me, s}];
    if (bytes > b.n) {
      if (b.p && b.pinned) {
        retired.push_back(b.p);      // a captured graph holds this address: keep it alive
      } else if (b.p) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipFree(b.p));
      }
      b = Slot{};
      void *p = nullptr;
      hipError_t e = hipMalloc(&p, bytes);
      if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(GFFT_ERR_NOMEM, "scratch allocation failed"); }
      HIP_TRY(e);
      b.p = p;
      b.n = bytes;
    }
    *out = b.p;
    return GFFT_OK;
  }
  // everything == false: the last plan of the process went away -- buffers no graph refers to are
  // freed; true: gfft_scratch_release(), the caller vouches that no captured graph will be replayed
  int release(bool everything) {
    std::lock_guard<std::mutex> lock(m);
    // (one device-wide synchronisation per device that holds a buffer: the stream handles in the keys may have been
    // destroyed since)
    const int here = current_device();
    int synced = -1;
    for (auto it = bufs.begin(); it != bufs.end();) {
      if (it->second.p && (everything || !it->second.pinned)) {
        if (it->first.dev != synced) {          // (keys are ordered by device)
          if (hipSetDevice(it->first.dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
          synced = it->first.dev;
        }
        (void)hipFree(it->second.p);
        it = bufs.erase(it);
      } else {
        ++it;
      }
    }
    if (synced >= 0 && synced != here && hipSetDevice(here) != hipSuccess) (void)hipGetLastError();
    if (everything) {
      if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
      for (void *p : retired) (void)hipFree(p);
      retired.clear();
    }
    return GFFT_OK;
  }
};

}  // namespace gfft

struct gfft_plan_s {
  int ndims = 0, kind = 0, precision = 0;
  std::vector<int64_t> sizes_in, sizes_out;
  std::vector<int> axes;
  std::vector<gfft::Pass> passes;
  size_t region_bytes[gfft::BUF_COUNT] = {0, 0, 0, 0, 0, 0, 0};   // WS / FS / AUX / RING / FS2 sizes
  double flops = 0, bytes = 0;
  int variant_rows = 0, variant_cols = 0, xcd_swizzle = 0;
  int tile_order = -1;                         // plan_fused3: PassDesc::order of the stand-alone strided passes; -1 = not a schedule that takes one
  bool fused3 = false;
  int mixv_variant = 0;                        // option mixv_variant at plan time (fft_mixv_*.hip: measured alternatives)
  int64_t ws_pitch = 0;                        // plan_fused3: entries between consecutive rows of the workspace
  int ws_tile = 0;                             // ... or: columns of a tile of its tile-major layout
  std::vector<int64_t> trunc;                  // gfft_plan_create_padded: kept entries per axis (else empty)
  std::vector<std::vector<hipEvent_t>> prof;   // per execute: events before pass 0 and after each pass
  std::vector<void *> device_allocs;            // small device buffers the plan owns (descriptors of fused launches)
  std::vector<gfft::Pass> alt;                       // stand-alone forms of the fused pairs (Pass::alt_first)
  unsigned id = 0;                              // what a voided fused launch reports (async_errors)
  int device = 0;                               // the device the plan's tables and descriptors live on
  std::atomic<bool> fused_off{false};           // a fused launch gave up a wait: the pairs run as stand-alone passes from now on
  std::atomic<bool> voided{false};              // ... and nobody has been told yet (poll_async_error)
  int async_slot = -1;                          // this plan's word of the host-visible table (async_errors; -1: none taken yet)
  gfft_plan_s();
  ~gfft_plan_s();
};

namespace gfft {

// the table of fused launches that gave up a wait (plan.cpp, above async_errors())
struct AsyncErrors {
  static constexpr int SLOTS = 256;
  std::mutex m;
  unsigned *flag = nullptr;                    // SLOTS pinned, device-visible words
  gfft_plan_s *owner[SLOTS] = {};              // the live plan each word belongs to (a plan takes one at its first fused launch)
  std::map<unsigned, gfft_plan_s *> live;
  std::vector<unsigned> orphans;               // ids of voided plans destroyed before anybody looked
  unsigned next_id = 1;
  unsigned *word() {
    if (!flag) {
      void *p = nullptr;
      if (hipHostMalloc(&p, SLOTS * sizeof(unsigned), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      flag = static_cast<unsigned *>(p);
      for (int i = 0; i < SLOTS; ++i) flag[i] = 0;
    }
    return flag;
  }
};

// ---- what the C surface calls into the planner (plan.cpp) ---------------------------------
Options &opts();
ScratchPool &scratch_pool();
AsyncErrors &async_errors();
extern std::atomic<int> g_live_plans;
int get_twiddles(int64_t n, int precision, const void **out);
void need(gfft_plan_s *pl, int buf, size_t bytes);
size_t align256(size_t b);
bool is_pow2(int64_t n);
int pow2_rows_nt(int64_t n, int precision);
bool regk_ok(int64_t n, int precision);
bool regk_c2c_ok(int64_t n, int precision, int mode);
bool real_half_mixv_ok(int64_t m);
bool fused_pad_ok(int64_t n_axis);
bool fused3_applicable(const gfft_plan_s *pl);
int plan_fused3(gfft_plan_s *pl);
int plan_line(gfft_plan_s *pl, const Line &L, bool top);
int plan_r2r_line(gfft_plan_s *pl, int64_t outer, int64_t n, int64_t inner, int kind, int src, int dst);
int build_pair2d(gfft_plan_s *pl, const gfft_iodim *cols, int64_t n2, const gfft_iodim *planes, bool inverse, int cols_first,
                 int in_blocks, int64_t in_block_stride, int out_blocks, int64_t out_block_stride, bool fused_only, bool *fused_out);
int build_pair2d_real(gfft_plan_s *pl, int64_t n1, int64_t n2, int64_t np, int64_t re_es, int64_t re_plane, int64_t cx_es,
                      int64_t cx_plane, int nb, int64_t bstride, bool inverse);
hipError_t run_pass(const gfft_plan_s *pl, const Pass &p, const PassDesc &d0, const void *in, void *out, double scale, hipStream_t s);
void fused_pairs_off(gfft_plan_s *pl);
int poll_async_error(gfft_plan_s *only);

// ---- rules both sides state ---------------------------------------------------------------
// smallest l with 2^l >= v (v >= 1); with is_pow2: the exponent of a block / tile count
inline int ilog2_ceil(int64_t v) { int l = 0; while (((int64_t)1 << l) < v) ++l; return l; }
// the fused 3/2-rule truncation (dir 1, on the store) / zero padding (dir 2, on the load) of a pass: n_keep entries stay
inline void set_truncation(PassDesc &d, int dir, int64_t n_keep) {
  d.tr_dir = dir;  d.tr_n = d.tr_N = (int)n_keep;  d.tr_even = (n_keep % 2 == 0) ? 1 : 0;
}

}  // namespace gfft
