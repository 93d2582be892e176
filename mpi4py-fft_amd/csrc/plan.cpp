// libgfft.so: the planner.  (The C ABI of include/gfft.h is api.cpp; what the two share is plan_internal.h.  The error state of
// the calling thread lives here, with gfft_last_error() beside it: api.cpp and the pseudo-spectral entry points in spectral.hip
// report errors, find the device and get scratch through the four functions gfft_internal.h declares from here.)
//
// The planner is the device-side counterpart of fftw_planxfftn() (mpi4py_fft/fftw/
// fftw_planxfftn.c:10-77): it turns (sizes, axes, kind) into one strided+batched 1-D pass per
// transformed axis -- {n, element stride, batch dims} exactly as the reference builds FFTW guru
// iodims (.c:25-47), but 64-bit -- and binds each pass to a kernel family:
//   * n = 2^k (16..4096), 3^b 2^k (48..3456) -> register-resident kernels (fft_pow2_impl.h; ROWS if
//                                       the axis is contiguous, else COLS)
//   * other n <= 4096 with small primes  -> fft_generic (LDS mixed radix)
//   * longer composite n                 -> four-step: two strided passes + fused twiddle
//   * anything else (large prime factors, long real transforms) -> Bluestein / complex embedding
//   * 3-D all-axes plans on one rank     -> plan_fused3: pass order + padded-pitch workspace
#include "plan_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

using namespace gfft;

namespace {

thread_local std::string g_last_error;
bool g_device_checked = false;

}  // namespace

extern "C" const char *gfft_last_error(void) { return g_last_error.c_str(); }

// what the entry points in api.cpp and spectral.hip share (declared in gfft_internal.h)
namespace gfft {

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? GFFT_ERR_NO_DEVICE : GFFT_ERR_HIP,
              std::string(what) + ": " + hipGetErrorString(e));
}

int check_device() {
  if (g_device_checked) return GFFT_OK;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(GFFT_ERR_NO_DEVICE, "no HIP device available (libgfft has no host fallback)");
  }
  g_device_checked = true;
  return GFFT_OK;
}

// ---- the planner: what plan_internal.h declares is called from api.cpp, the rest stays in this file -----------------
Options &opts() {
  static Options o;
  return o;
}

// ---- twiddle tables (device resident, shared by plans) ------------------------------------
// (per device: the key's precision slot also carries the ordinal of the device the table lives on)
namespace {
int dev_prec(int precision) { return precision + (current_device() << 8); }
std::mutex g_tw_mutex;
std::map<std::tuple<int64_t, int, int>, void *> g_tw_cache;       // (n, precision + device, test-hook signature) -> W_n^k, k<n
std::map<std::pair<int64_t, int>, BigTw> g_bigtw_cache;     // (big_n, precision)

// exp(-2 pi i k / n) for k in [k0, k0 + count*step) step `step`, in long double, stored as `precision`
int upload_twiddles(int64_t n, int64_t step, int64_t count, int precision, void **out, int64_t wrong_index = -1, double wrong_by = 0) {
  const long double w = -2.0L * 3.14159265358979323846264338327950288L / (long double)n;
  std::vector<unsigned char> host((size_t)count * 2 * precision);
  for (int64_t j = 0; j < count; ++j) {
    const int64_t k = (j * step) % n;
    // reduce to the first octant for accuracy
    long double c, s;
    {
      const long double a = w * (long double)k;
      c = cosl(a);
      s = sinl(a);
      if (4 * k == n) { c = 0; s = -1; }
      else if (2 * k == n) { c = -1; s = 0; }
      else if (4 * k == 3 * n) { c = 0; s = 1; }
      else if (k == 0) { c = 1; s = 0; }
    }
    if (j == wrong_index) c += (long double)wrong_by;          // (test hook, Options::debug_tw_exp)
    if (precision == 8) {
      double *p = reinterpret_cast<double *>(host.data()) + 2 * j;
      p[0] = (double)c;
      p[1] = (double)s;
    } else {
      float *p = reinterpret_cast<float *>(host.data()) + 2 * j;
      p[0] = (float)c;
      p[1] = (float)s;
    }
  }
  void *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size()));
  HIP_TRY(hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice));
  *out = d;
  return GFFT_OK;
}
}  // namespace

int get_twiddles(int64_t n, int precision, const void **out) {
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  const int e = (opts().debug_tw_len == 0 || opts().debug_tw_len == n) ? opts().debug_tw_exp : 0;
  const int64_t wrong = e > 0 ? ((int64_t)opts().debug_tw_index % n + n) % n : -1;
  auto key = std::make_tuple(n, dev_prec(precision), e > 0 ? (int)(wrong * 64 + (e & 63)) + 1 : 0);
  auto it = g_tw_cache.find(key);
  if (it == g_tw_cache.end()) {
    void *d = nullptr;
    int rc = upload_twiddles(n, 1, n, precision, &d, wrong, e > 0 ? std::pow(10.0, -e) : 0.0);
    if (rc) return rc;
    it = g_tw_cache.emplace(key, d).first;
  }
  *out = it->second;
  return GFFT_OK;
}

static int get_bigtw(int64_t big_n, int precision, BigTw *out) {
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  auto key = std::make_pair(big_n, dev_prec(precision));
  auto it = g_bigtw_cache.find(key);
  if (it == g_bigtw_cache.end()) {
    int L = 0;
    while (((int64_t)1 << (2 * L)) < big_n) ++L;     // 2^L ~ sqrt(big_n)
    const int64_t lo_n = (int64_t)1 << L;
    const int64_t hi_n = (big_n + lo_n - 1) / lo_n;
    BigTw t{nullptr, nullptr, L};
    int rc = upload_twiddles(big_n, 1, lo_n < big_n ? lo_n : big_n, precision, &t.lo);
    if (rc) return rc;
    rc = upload_twiddles(big_n, lo_n, hi_n, precision, &t.hi);
    if (rc) return rc;
    it = g_bigtw_cache.emplace(key, t).first;
  }
  *out = it->second;
  return GFFT_OK;
}

bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }

/* threads per line (NT = n / R) of the power-of-two ROW kernels, as the tables in fft_pow2_f64.hip /
 * fft_pow2_f32.hip instantiate them (default variants); launch_pow2_one re-checks at launch */
int pow2_rows_nt(int64_t n, int precision) {
  if (!is_pow2(n) || n < 16 || n > 4096) return 0;
  if (n <= 32) return 4;
  if (n == 64) return 8;
  if (n == 128) return 16;
  if (n == 256) return precision == 8 ? 32 : 16;
  if (n <= 1024) return 64;
  return (int)(n / 16);
}

// lengths served by the register-resident kernels: 2^k (16..4096), 3^b 2^k (48..3456), 5^c 2^k (20..4000)
bool regk_ok(int64_t n, int precision) {
  if (opts().force_generic) return false;
  if (n > 4096) return false;
  if (mix3_supported((int)n) || mix5_supported((int)n)) return true;
  return precision == 8 ? pow2_supported_f64((int)n) : pow2_supported_f32((int)n);
}

// ... plus the lengths that have plain COMPLEX one-pass kernels only (3 x 5 x 2^k and neighbours, fft_mixv_*.hip: no real
// modes, no fused truncation, no four-step twiddle, no exchange-buffer layouts): natural-layout c2c lines and the complex
// passes of the one-rank 3-D schedule take them; everything else keeps the paths it had
bool regk_c2c_ok(int64_t n, int precision, int mode) {
  (void)precision;
  return !opts().force_generic && opts().mixv && mode == MODE_C2C && n <= 4096 && mixv_supported((int)n);
}

// ... and packed-real rows of twice such a length (complex length m = n / 2): plain rows only
bool real_half_mixv_ok(int64_t m) { return !opts().force_generic && opts().mixv && m <= 4096 && mixv_supported((int)m); }

// lengths whose kernels carry the fused 3/2-rule truncation / zero-padding adapters: every register-kernel
// length except 5^c 2^k, whose adapters only a `make VARIANTS=1` library instantiates (fft_pow2_impl.h
// TF_NO_TRUNC, kFusedPadMix5) -- plans on those lengths keep the separate gfft_truncate / gfft_pad
// kernels.  `n_axis`: transformed length of a complex axis, or the COMPLEX length (half) of a packed-real row.
bool fused_pad_ok(int64_t n_axis) {
#ifdef GFFT_VARIANTS
  // (a `make VARIANTS=1` library instantiates the 5^c 2^k adapters; the unequal-width lengths not divisible by 3 have none in ANY build)
  return !(n_axis <= 4096 && mixv_supported((int)n_axis) && n_axis % 3 != 0);
#else
  // (the unequal-width stage kernels carry the adapters on lengths divisible by 3: what the 3/2-rule makes of 5 x 2^k, 7 x 2^k ...)
  return !(n_axis <= 4096 && (mix5_supported((int)n_axis) || (mixv_supported((int)n_axis) && n_axis % 3 != 0)));
#endif
}

static bool factorize(int64_t n, Factors *f, int max_prime) {
  f->count = 0;
  auto push = [&](int r) { if (f->count < 24) f->r[f->count++] = r; };
  while (n % 4 == 0) { push(4); n /= 4; }
  while (n % 2 == 0) { push(2); n /= 2; }
  while (n % 3 == 0) { push(3); n /= 3; }
  for (int64_t p = 5; p * p <= n; p += 2)
    while (n % p == 0) { push((int)p); n /= p; }
  if (n > 1) push((int)n);
  for (int i = 0; i < f->count; ++i)
    if (f->r[i] > max_prime) return false;
  if (f->count == 0) { f->count = 1; f->r[0] = 1; }
  return true;
}

// the generic kernel evaluates a prime radix r by definition, O(r^2) per butterfly: fine for the
// small odd primes of everyday sizes, hopeless for big ones -> Bluestein above this
constexpr int GENERIC_MAX_PRIME = 61;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

ScratchPool &scratch_pool() {
  static ScratchPool p;
  return p;
}
// plans alive: when the last one goes the shared workspaces go with it (a 1024^3 plan leaves 16 GiB)
std::atomic<int> g_live_plans{0};

int scratch_get(hipStream_t s, size_t bytes, void **out) { return scratch_pool().get(s, bytes, out); }

// ---- fused launches that gave up a wait (fft_pow2_impl.h fused_give_up) --------------------------------
// The kernel writes the plan's id into the plan's OWN word of a small table of pinned host words (taken at the plan's first
// fused launch, given back when the plan is destroyed: two live plans never share one); the library scans the table on entry to gfft_execute, in
// gfft_plan_status() and in gfft_async_error().  A plan named there switches its pairs to stand-alone passes and carries
// the error until it is reported ONCE: by that plan's own next gfft_execute (which enqueues nothing), by
// gfft_plan_status(plan), or by gfft_async_error() -- whichever looks first.  Other plans are not refused: the results of
// the voided plan's last execution are invalid, everything else is untouched.
AsyncErrors &async_errors() {
  static AsyncErrors a;
  return a;
}
// this plan runs its pairs as stand-alone passes from now on: grow the scratch regions that only that form needs
void fused_pairs_off(gfft_plan_s *pl) {
  pl->fused_off = true;
  for (const Pass &p : pl->passes)
    if (p.kind == PK_FUSED2 && p.alt_buf >= 0 && p.alt_bytes > pl->region_bytes[p.alt_buf]) pl->region_bytes[p.alt_buf] = p.alt_bytes;
}
// move what the kernels wrote since the last look into the plans (a.m held by the caller)
static void collect_async_errors(AsyncErrors &a) {
  if (!a.flag) return;
  for (int i = 0; i < AsyncErrors::SLOTS; ++i) {
    // (a plain look first -- this runs on entry to every gfft_execute --, then ONE exchange, not load-then-store: a word written
    // between the two would be lost)
    if (!__atomic_load_n(a.flag + i, __ATOMIC_RELAXED)) continue;
    const unsigned id = __atomic_exchange_n(a.flag + i, 0u, __ATOMIC_ACQ_REL);
    if (!id) continue;
    auto it = a.live.find(id);
    if (it == a.live.end()) { a.orphans.push_back(id); continue; }
    gfft_plan_s *pl = it->second;
    fused_pairs_off(pl);
    pl->voided = true;
  }
}
static int report_voided(unsigned id) {
  char msg[320];
  snprintf(msg, sizeof msg, "a fused launch of plan #%u waited longer than %d ms for another workgroup and gave up (device shared or stalled?): "
           "the results of that plan's last execution are INVALID; the plan runs its pass pairs as stand-alone launches from now on", id,
           opts().fuse2_wait_ms);
  return fail(GFFT_ERR_VOIDED, msg);
}
// `only`: report this plan's pending event (if any); nullptr: report any pending event
int poll_async_error(gfft_plan_s *only) {
  AsyncErrors &a = async_errors();
  if (!a.flag) return GFFT_OK;
  std::lock_guard<std::mutex> lock(a.m);
  collect_async_errors(a);
  if (only) {
    if (!only->voided.exchange(false)) return GFFT_OK;
    return report_voided(only->id);
  }
  for (auto &kv : a.live)
    if (kv.second->voided.exchange(false)) return report_voided(kv.first);
  if (!a.orphans.empty()) {
    const unsigned id = a.orphans.back();
    a.orphans.pop_back();
    return report_voided(id);
  }
  return GFFT_OK;
}
}  // namespace gfft
gfft_plan_s::gfft_plan_s() {
  device = current_device();
  AsyncErrors &a = async_errors();
  std::lock_guard<std::mutex> lock(a.m);
  id = a.next_id++;
  if (!a.next_id) a.next_id = 1;
  a.live[id] = this;
}
gfft_plan_s::~gfft_plan_s() {
  {
    AsyncErrors &a = async_errors();
    std::lock_guard<std::mutex> lock(a.m);
    if (a.flag && async_slot >= 0) {
      // (a launch of this plan may have voided itself since the last look: its word goes with the slot)
      if (__atomic_exchange_n(a.flag + async_slot, 0u, __ATOMIC_ACQ_REL) == id) voided = true;
      a.owner[async_slot] = nullptr;
    }
    if (voided.exchange(false)) a.orphans.push_back(id);      // destroyed before anybody looked: still reported, by gfft_async_error
    a.live.erase(id);
  }
  for (void *q : device_allocs) (void)hipFree(q);
}

namespace gfft {

void need(gfft_plan_s *pl, int buf, size_t bytes) {
  if (bytes > pl->region_bytes[buf]) pl->region_bytes[buf] = bytes;
}

namespace {

// Row pitches of the scratch arrays (workspace, four-step intermediate, hand-off slots), in entries of esz bytes.
// Rule 1: +256 B when the pitch would be a multiple of 2 KiB (rows a power of two apart alias the memory channels).
int64_t pitch_off_2k(int64_t P, int64_t esz) { return (P * esz) % 2048 == 0 ? P + 256 / esz : P; }
// Rule 2, for rows of whole 128-byte lines (P a multiple of 128 / esz, and it stays one): off the multiples of 2 KiB
// ... and never 129 x 2^k entries: the far stride of the workspace is a power of two times P, and with P = 129 x 2^k
// the rows a far-axis tile walks lie k (2^7 + 1) 2^j bytes apart -- the one multiplier found so far that the address
// hash of the memory channels folds onto itself (row k and row k + 2^7 j share their channel).  Measured (round 5,
// tools/ab_combo_probe.py ws_plane_skew, profiles/r05_ab_pitch129.txt), far-axis pass alone, same arrays:
// (1024,1024,2048) r2c f64 [1025-wide rows, P = 1032] 11.6 -> 7.2 ms; (512,1024,2048) c128 [P = 2064] 14.0 -> 6.4 ms;
// (2048,512,2048) r2c f64 18.0 -> 7.8 ms; (1024,1024,4096) r2c f32 [2049-wide, P = 2064] 14.0 -> 8.5 ms; pitches of
// 17 / 33 / 65 / 257 x 2^k entries (every other BASELINE-sized shape) are level with or without a skew.
int64_t pitch_off_129(int64_t P, int64_t esz) {
  auto odd = [](int64_t x) { while (x && !(x & 1)) x >>= 1; return x; };
  while (odd(P) == 129 || (P * esz) % 2048 == 0) P += 128 / esz;
  return P;
}

// Slots of the hand-off ring and planes the producer runs ahead (options fuse2_ring / fuse2_lag, else automatic); false:
// this launch has too few planes for a ring on which the pair pays.
// How far the producer runs ahead is a matter of BYTES, not planes: ~96 MiB of lead, twice that of ring (the Infinity
// Cache holds 256 MiB) -- 6 / 12 planes of 16 MiB (complex128, n = 1024: the optimum of the round-3 sweeps), 12 / 24
// planes of 8 MiB (complex64: with 6 / 12 the pair LOSES, 21.1 -> 21.9 ms per 1024^3 step, with 12 / 24 it gains, ->
// 18.9 ms; profiles/r04_ab_fuse2_f32.txt), 24 / 48 planes of 4 MiB (complex128 n = 512: 16 / 32 +11 %, 24 / 48 -11 %).
bool fused2_ring(int precision, int n_a, int n_b, int64_t slot_bytes, int planes, int *ring_out, int *lag_out) {
  // auto: 12 slots with the producer 6 planes ahead where there are planes enough, else 8 / 4.  Swept on one box, plans
  // alternating on the same arrays (tools/fused2_ring_sweep.py, profiles/r03_fused2_ring_sweep_final.txt): 1024^3
  // complex128 per step 34.3 (8 / 4) -> 32.4 (12 / 6), 32.2 (14 / 7), 31.8 (13 / 6, 11 / 6); lag 3 or ring 6: 37.9;
  // C2 0.748 -> 0.710 ms (16 / 8: 0.70).  (Before the row tiles lost their barriers 8 / 4 was the optimum: a
  // faster consumer wants the producer further ahead.)
  int ring = opts().fuse2_ring, lag = opts().fuse2_lag;
  if (ring <= 0) {
    int64_t ahead = (((int64_t)96 << 20) + slot_bytes - 1) / (slot_bytes > 0 ? slot_bytes : 1);
    ahead = ahead < 4 ? 4 : (ahead > 32 ? 32 : ahead);
    ring = 2 * (int)ahead;
    // too few planes for that: the complex128 n = 1024 pairs still pay on a shorter ring (8 / 4: 34.3 against 39.9 ms
    // unfused, round 3); the others LOSE with less lead than this and stay unfused
    if (planes < 2 * ring) {
      if (!(precision == GFFT_F64 && (n_a == 1024 || n_b == 1024))) return false;      // (the real fp64 pairs: 12 / 6 ... 24 / 12 level)
      while (ring > 8 && planes < 2 * ring) ring -= 2;
    }
  }
  if (lag <= 0) lag = ring / 2;
  if (planes < 2 * ring || lag < 1 || ring <= lag) return false;
  *ring_out = ring;
  *lag_out = lag;
  return true;
}

// The hand-off protocol of the fused pairs leans on gfx94x / gfx950 specifics (fused2_pair): elsewhere the pairs stay off.
bool fused2_arch_ok() {
  static int arch_ok[kMaxDevices] = {};          // 0 unknown, 1 yes, -1 no
  const int dev = current_device();
  if (!arch_ok[dev]) {
    hipDeviceProp_t prop;
    arch_ok[dev] = -1;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
      if (!strncmp(prop.gcnArchName, "gfx942", 6) || !strncmp(prop.gcnArchName, "gfx950", 6)) arch_ok[dev] = 1;
    } else {
      (void)hipGetLastError();
    }
  }
  return arch_ok[dev] > 0;
}

// Whether a kernel pair exists for (precision, kind, n_a, n_b) on `planes` planes of slot_bytes each, and its ring: everything
// that can be known without the descriptors.  make_fused2 starts from it, and plan_fused3 asks it BEFORE it lays the workspace
// out for a pair.  pair == nullptr: no pair.
PairChoice fused2_pair(int precision, int kind, int n_a, int n_b, int64_t slot_bytes, int planes) {
  // The hand-off protocol leans on gfx94x / gfx950 specifics: raw-buffer cache policy sc0 | sc1 = system scope (written
  // through / never served from a stale L2 line), stores counted by vmcnt -- so that s_waitcnt(0) means "write-through
  // acknowledged" --, relaxed agent-scope atomics as the only ordering.  On a target with another memory model (a
  // separate store counter, other policy bits) the pairs stay off: the stand-alone passes are always correct.
  PairChoice c;
  if (!fused2_arch_ok()) return c;
  if (!opts().fuse2 || !((opts().fuse2_kinds >> kind) & 1)) return c;
  // (complex64 pairs are on by default since round 4 -- option fuse2_f32 = 1, profiles/r04_ab_fuse2_f32.txt; the real fp32
  // pairs measured level to slightly slower than their stand-alone passes -- 1024^3 r2c f32 per step 11.53 ms unfused, 11.58
  // with both pairs, 11.78 with the r2c pair alone, 11.42 with the c2r pair alone, profiles/r04_real_pairs_f32.txt -- and
  // need fuse2_f32 = 2)
  if (precision == GFFT_F32 && (!opts().fuse2_f32 || (fused_kind_real(kind) && opts().fuse2_f32 < 2))) return c;
  if (!fused2_ring(precision, n_a, n_b, slot_bytes, planes, &c.ring, &c.lag)) return c;
  c.pair = fused2_select(precision, kind, opts().fuse2, n_a, n_b);
  return c;
}

// Turn two consecutive passes A -> B into one fused launch when a kernel pair exists: dA / dB are the passes
// cut down to one plane, the plane strides say where plane p starts on A's input and B's output side.
bool make_fused2(gfft_plan_s *pl, int kind, const Pass &a, const Pass &b, const PassDesc &dA, const PassDesc &dB, int planes,
                 int64_t a_in_plane, int64_t b_out_plane, int64_t slot_bytes, Pass *out) {
  const PairChoice c = fused2_pair(pl->precision, kind, dA.n, dB.n, slot_bytes, planes);
  if (!c.pair) return false;
  const int ta = (int)c.pair->tiles_a(dA), tb = (int)c.pair->tiles_b(dB);
  if (ta < 1 || tb < 1) return false;
  // (hand-off accesses carry 32-bit byte offsets inside a slot; tickets are 32-bit)
  if (slot_bytes >= ((int64_t)1 << 31) || (double)planes * (ta + tb) >= 1.0e9) return false;     // (tickets < 2^30: a launch that gives up pushes the counter 2^31 on)
  Pass f = a;
  f.kind = PK_FUSED2;
  f.fused_kind = kind;
  f.pair = c.pair;
  f.d = dA;
  f.d2 = dB;
  f.src = a.src;
  f.dst = b.dst;
  f.carries_scale = false;
  f.fused.planes = planes;
  f.fused.tiles_a = ta;
  f.fused.tiles_b = tb;
  f.fused.ring = c.ring;
  f.fused.lag = c.lag;
  f.fused.defer = 0;      // an A tile's counter is settled at the end of the tile (1 / 2: behind the next tile's loads / the next ticket's poll -- measured, not kept)
  f.fused.group = 1;      // one tile per ticket (groups of 2 / 4 measured level to slower, profiles/r03_ab_fuse2_group.txt)
  f.fused.a_in_plane = a_in_plane;
  f.fused.b_out_plane = b_out_plane;
  f.fused.slot_bytes = (int64_t)align256((size_t)slot_bytes);
  f.fused.ctr = nullptr;
  f.fused.wait_ticks = 0;            // (filled in at execution: option fuse2_wait_ms)
  f.fused.plan_id = pl->id;
  f.fused.host_flag = nullptr;
  f.fused.debug = 0;
  for (const Pass *q : {&a, &b})
    for (int side : {q->src, q->dst})
      if (side >= BUF_WS && side != BUF_RING) f.alt_buf = side;     // (at most one scratch region: WS of the 3-D schedule, FS of a four-step pair)

  size_t ctr_bytes = align256((size_t)(16 + 2 * planes) * sizeof(unsigned));
#ifdef GFFT_FUSE2_TRACE
  ctr_bytes += 256 + (size_t)1024 * 96 * 16 * sizeof(unsigned long long);       // (fft_pow2_impl.h, GFFT_TRACE_STAMP)
#endif
  // the kernel reads the two descriptors from device memory (the scale factors travel as kernel arguments)
  const PassDesc both[2] = {f.d, f.d2};
  void *dev = nullptr;
  if (hipMalloc(&dev, sizeof both) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (hipMemcpy(dev, both, sizeof both, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(dev); return false; }
  pl->device_allocs.push_back(dev);
  f.dev_descs = static_cast<PassDesc *>(dev);
  // (nothing of the plan is touched before the pair is certain)
  need(pl, BUF_RING, (size_t)c.ring * (size_t)f.fused.slot_bytes + ctr_bytes);
  f.alt_first = (int)pl->alt.size();
  pl->alt.push_back(a);
  pl->alt.push_back(b);
  *out = f;
  return true;
}

PassDesc natural_desc(const Line &L) {
  PassDesc d{};
  d.n = (int)L.n;
  d.mode = L.mode;
  d.conj_in = L.inverse ? 1 : 0;
  d.conj_out = (L.inverse && L.mode != MODE_C2R) ? 1 : 0;
  d.batch = L.outer * L.inner;
  d.mid = 1;
  d.inner = L.inner;
  d.in_os = L.nin * L.inner;
  d.in_is = 1;
  d.in_es = L.inner;
  d.out_os = L.nout * L.inner;
  d.out_is = 1;
  d.out_es = L.inner;
  d.scale = 1.0;
  return d;
}

// Real lines along a contiguous axis, even length: the packed-real form (MODE_R2C_H / MODE_C2R_H).
bool real_half_ok(const Line &L, int prec) {
  (void)prec;
  return !opts().force_generic && (L.mode == MODE_R2C || L.mode == MODE_C2R) &&
         L.inner == 1 && L.n % 2 == 0 && L.n / 2 <= 4096 &&
         (real_half_supported((int)(L.n / 2)) || real_half_mix_supported((int)(L.n / 2)) || real_half_mixv_ok(L.n / 2)) && L.outer < ((int64_t)1 << 31);
}

// natural_desc(L) restated for the packed-real form: d.n = complex length, real side in pairs
void half_desc(PassDesc *d, const Line &L) {
  const int64_t m = L.n / 2;
  d->n = (int)m;
  d->mode = L.mode == MODE_R2C ? MODE_R2C_H : MODE_C2R_H;
  d->conj_in = 0;
  d->conj_out = L.mode == MODE_C2R ? 1 : 0;     // inverse by conjugation: the pre-pass conjugates
  d->in_os = L.mode == MODE_R2C ? m : m + 1;
  d->out_os = L.mode == MODE_R2C ? m + 1 : m;
  d->in_es = d->out_es = 1;
  d->in_is = d->out_is = 1;
}

// ---- four-step for long composite lengths: n = n1 * n2 (complex) ---------------------------
int plan_fourstep(gfft_plan_s *pl, const Line &L, int64_t n1, int64_t n2) {
  const int prec = pl->precision;
  const int64_t esz = 2 * prec, n = L.n, inner = L.inner, outer = L.outer;
  BigTw bt;
  int rc = get_bigtw(n, prec, &bt);
  if (rc) return rc;
  // The intermediate tmp[o][i2][k1][i] lives in the FS region with its i2-stride S2 padded off
  // the power of two (same channel-aliasing argument as the 3-D workspace).
  const int64_t S2 = pitch_off_2k(n1 * inner, esz);
  Pass a, b;
  // step 1: length-n1 transforms over i1 (stride n2*inner) for every (o, i2, i); the store
  // applies W_n^(i2*k1) and writes transposed-within-row
  a.d = natural_desc(L);
  a.d.n = (int)n1;
  a.d.batch = outer * n2 * inner;
  a.d.mid = n2;
  a.d.inner = inner;
  a.d.in_os = n * inner;  a.d.in_ms = inner;  a.d.in_is = 1;  a.d.in_es = n2 * inner;
  a.d.out_os = n2 * S2;   a.d.out_ms = S2;    a.d.out_is = 1; a.d.out_es = inner;
  a.d.conj_in = L.inverse ? 1 : 0;
  a.d.conj_out = 0;
  a.d.tw_hi = bt.hi;  a.d.tw_lo = bt.lo;  a.d.tw_L = bt.L;  a.d.big_n = n;
  a.src = L.src;
  a.dst = BUF_FS;
  a.logical_first = true;
  // step 2: length-n2 transforms over i2 (stride S2) for every (o, k1, i); natural output
  b.d = natural_desc(L);
  b.d.n = (int)n2;
  b.d.batch = outer * n1 * inner;
  b.d.mid = 1;
  b.d.inner = n1 * inner;
  b.d.in_os = n2 * S2;   b.d.in_is = 1;  b.d.in_es = S2;
  b.d.out_os = n * inner; b.d.out_is = 1; b.d.out_es = n1 * inner;
  b.d.conj_in = 0;
  b.d.conj_out = L.inverse ? 1 : 0;
  b.src = BUF_FS;
  b.dst = L.dst;
  const int gmax = generic_max_n(prec);
  for (Pass *q : {&a, &b}) {
    const int64_t m = q->d.n;
    if (regk_ok(m, prec)) {
      q->regk = true;
      q->cols = true;
    } else if (!(m <= gmax && factorize(m, &q->f, GENERIC_MAX_PRIME))) {
      return fail(GFFT_ERR_UNSUPPORTED, "four-step factor not plannable");
    }
    rc = get_twiddles(m, prec, &q->d.tw);
    if (rc) return rc;
  }
  // Both passes in one persistent launch, a signal's intermediate handed over inside the Infinity Cache
  // (FUSED_FOURSTEP): plane = one signal, slot = its [n2][S2] intermediate.
  if (a.regk && b.regk && inner == 1 && outer < ((int64_t)1 << 30)) {
    Pass f;
    {
      // FUSED_FOURSTEP_ROWS: the intermediate the other way round, tmp[k1][i2] (rows of n2 entries, pitch S1): the
      // first pass stores its 16 columns i2 .. i2 + 15 side by side where they are, the second reads rows
      const int64_t S1 = pitch_off_2k(n2, esz);
      PassDesc dA = a.d, dB = b.d;
      dA.batch = n2;
      dA.out_os = n1 * S1;  dA.out_ms = 1;  dA.out_is = 1;  dA.out_es = S1;
      dB.batch = n1;
      dB.mid = n1;  dB.inner = 1;
      dB.in_os = n1 * S1;  dB.in_ms = S1;  dB.in_is = 1;  dB.in_es = 1;
      dB.out_os = n;  dB.out_ms = 1;  dB.out_is = 1;  dB.out_es = n1;
      if (make_fused2(pl, FUSED_FOURSTEP_ROWS, a, b, dA, dB, (int)outer, n * esz, n * esz, n1 * S1 * esz, &f)) {
        f.alt_bytes = (size_t)outer * n2 * S2 * esz;
        pl->passes.push_back(f);
        return GFFT_OK;
      }
    }
    PassDesc dA = a.d, dB = b.d;
    dA.batch = n2;           // (o, i2, i) with o = 0
    dB.batch = n1;
    if (make_fused2(pl, FUSED_FOURSTEP, a, b, dA, dB, (int)outer, n * esz, n * esz, n2 * S2 * esz, &f)) {
      f.alt_bytes = (size_t)outer * n2 * S2 * esz;
      pl->passes.push_back(f);
      return GFFT_OK;
    }
  }
  need(pl, BUF_FS, (size_t)outer * n2 * S2 * esz);
  pl->passes.push_back(a);
  pl->passes.push_back(b);
  return GFFT_OK;
}

// Pick n1*n2 = n with both factors plannable in one pass; prefers the register-kernel sizes.
bool split_fourstep(int64_t n, int prec, int64_t *n1, int64_t *n2) {
  const int gmax = generic_max_n(prec);
  if (n > ((int64_t)1 << 24)) return false;
  if (is_pow2(n)) {
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    *n1 = (int64_t)1 << ((lg + 1) / 2);
    *n2 = n / *n1;
    return *n1 <= 4096;
  }
  int64_t best = 0;
  for (int64_t a = (int64_t)std::sqrt((double)n); a >= 2; --a) {
    if (n % a) continue;
    const int64_t b = n / a;
    Factors fa, fb;
    const bool oka = regk_ok(a, prec) || (a <= gmax && factorize(a, &fa, GENERIC_MAX_PRIME));
    const bool okb = regk_ok(b, prec) || (b <= gmax && factorize(b, &fb, GENERIC_MAX_PRIME));
    if (!oka || !okb) continue;
    if (regk_ok(a, prec) && regk_ok(b, prec)) { best = a; break; }
    if (!best) best = a;
  }
  if (!best) return false;
  *n1 = n / best;
  *n2 = best;
  return true;
}

// ---- lengths beyond 2^24: n = n1 * n2 with n2 a four-step (or single-pass) length again ------------------------------
// FFTW plans any length (/root/reference/mpi4py_fft/fftw/fftw_planxfftn.c:52-75).  One more level of the same
// decomposition: the strided pass of length n1 with the twiddle W_n^(i2 k1) on its store leaves tmp[o][i2][k1][i] --
// which IS the natural layout [outer][n2][inner'] of a batch of lines of length n2 with inner' = n1 * inner, and the
// result of transforming those lines in place of i2, out[o][k2][k1][i], is the natural order k = k2 n1 + k1 of the long
// transform.  So the rest is plan_line on that batch (a four-step transform with inner > 1: two passes through FS):
// three HBM round trips in all, the intermediate of this level in its own region (FS2).  Inverse: conj . forward . conj
// level by level -- this pass conjugates on load AND on store, the inner line conjugates again on its load.
int plan_long(gfft_plan_s *pl, const Line &L, int64_t n1, int64_t n2) {
  const int prec = pl->precision;
  const int64_t esz = 2 * prec, n = L.n, inner = L.inner, outer = L.outer;
  BigTw bt;
  int rc = get_bigtw(n, prec, &bt);
  if (rc) return rc;
  const int64_t S2 = n1 * inner;
  Pass a;
  a.d = natural_desc(L);
  a.d.n = (int)n1;
  a.d.batch = outer * n2 * inner;
  a.d.mid = n2;
  a.d.inner = inner;
  a.d.in_os = n * inner;  a.d.in_ms = inner;  a.d.in_is = 1;  a.d.in_es = n2 * inner;
  a.d.out_os = n2 * S2;   a.d.out_ms = S2;    a.d.out_is = 1; a.d.out_es = inner;
  a.d.conj_in = L.inverse ? 1 : 0;
  a.d.conj_out = L.inverse ? 1 : 0;
  a.d.tw_hi = bt.hi;  a.d.tw_lo = bt.lo;  a.d.tw_L = bt.L;  a.d.big_n = n;
  a.src = L.src;
  a.dst = BUF_FS2;
  a.logical_first = true;
  a.regk = true;
  a.cols = true;
  rc = get_twiddles(n1, prec, &a.d.tw);
  if (rc) return rc;
  need(pl, BUF_FS2, (size_t)outer * n * inner * esz);
  pl->passes.push_back(a);
  const Line rest{outer, S2, n2, n2, n2, MODE_C2C, L.inverse, BUF_FS2, L.dst};
  return plan_line(pl, rest, false);
}

// n1 for plan_long: a register-kernel length whose cofactor plan_line takes in one or two passes; powers of two split
// three ways as evenly as the tables allow (2^30 = 1024 x (1024 x 1024))
bool split_long(int64_t n, int prec, int64_t *n1) {
  if (n <= ((int64_t)1 << 24) || n >= ((int64_t)1 << 31)) return false;
  int64_t t1 = 0, t2 = 0;
  if (is_pow2(n)) {
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    *n1 = (int64_t)1 << (lg - 2 * (lg / 3));
    return true;
  }
  for (int64_t a = 4096; a >= 16; --a) {
    if (n % a || !regk_ok(a, prec)) continue;
    const int64_t b = n / a;
    if (b > ((int64_t)1 << 24)) break;
    if (regk_ok(b, prec) || split_fourstep(b, prec, &t1, &t2)) { *n1 = a; return true; }
  }
  return false;
}

// ---- embedding fallbacks: Bluestein, and real transforms beyond the single-pass limit --------
// Both copy the lines into a complex AUX array [outer][Lw][inner], transform there, and extract.
//   real-as-complex: Lw = n, the complex engine is whatever plan_line picks for length n
//   Bluestein      : Lw = M = 2^k >= 2n-1; x_j w_j -> FFT_M -> * B -> IFFT_M -> * w_k / M,
//                    w_j = exp(-i pi j^2 / n), B = FFT_M(conj chirp, wrapped)
std::map<std::pair<int64_t, int>, std::pair<void *, void *>> g_blue_cache;   // (n, prec) -> (chirp, B)

void host_fft_pow2(std::vector<long double> &re, std::vector<long double> &im) {
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  const long double PI = 3.14159265358979323846264338327950288L;
  for (size_t len = 2; len <= n; len <<= 1) {
    for (size_t k = 0; k < len / 2; ++k) {
      const long double a = -2.0L * PI * (long double)k / (long double)len;
      const long double wr = cosl(a), wi = sinl(a);
      for (size_t i = k; i < n; i += len) {
        const size_t j = i + len / 2;
        const long double tr = re[j] * wr - im[j] * wi, ti = re[j] * wi + im[j] * wr;
        re[j] = re[i] - tr; im[j] = im[i] - ti;
        re[i] += tr;        im[i] += ti;
      }
    }
  }
}

int get_bluestein(int64_t n, int64_t M, int prec, const void **chirp, const void **B) {
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  auto key = std::make_pair(n, dev_prec(prec));
  auto it = g_blue_cache.find(key);
  if (it == g_blue_cache.end()) {
    const long double PI = 3.14159265358979323846264338327950288L;
    std::vector<long double> cr(n), ci(n), br(M, 0.0L), bi(M, 0.0L);
    for (int64_t j = 0; j < n; ++j) {
      const int64_t q = (j * j) % (2 * n);                  // exact phase reduction
      const long double a = PI * (long double)q / (long double)n;
      cr[j] = cosl(a);
      ci[j] = -sinl(a);                                      // w_j = exp(-i pi j^2 / n)
      br[j] = cr[j];
      bi[j] = -ci[j];                                        // b_j = conj(w_j)
      if (j) { br[M - j] = br[j]; bi[M - j] = bi[j]; }
    }
    host_fft_pow2(br, bi);
    auto upload = [&](const std::vector<long double> &xr, const std::vector<long double> &xi, void **out) -> int {
      std::vector<unsigned char> h(xr.size() * 2 * prec);
      for (size_t j = 0; j < xr.size(); ++j) {
        if (prec == 8) { ((double *)h.data())[2 * j] = (double)xr[j]; ((double *)h.data())[2 * j + 1] = (double)xi[j]; }
        else { ((float *)h.data())[2 * j] = (float)xr[j]; ((float *)h.data())[2 * j + 1] = (float)xi[j]; }
      }
      HIP_TRY(hipMalloc(out, h.size()));
      HIP_TRY(hipMemcpy(*out, h.data(), h.size(), hipMemcpyHostToDevice));
      return GFFT_OK;
    };
    void *dc = nullptr, *db = nullptr;
    int rc = upload(cr, ci, &dc);
    if (rc) return rc;
    rc = upload(br, bi, &db);
    if (rc) return rc;
    it = g_blue_cache.emplace(key, std::make_pair(dc, db)).first;
  }
  *chirp = it->second.first;
  *B = it->second.second;
  return GFFT_OK;
}

int plan_embedded(gfft_plan_s *pl, const Line &L, bool bluestein) {
  const int prec = pl->precision;
  const int64_t esz = 2 * prec;
  int64_t Lw = L.n;
  const void *chirp = nullptr, *B = nullptr;
  if (bluestein) {
    Lw = 1;
    while (Lw < 2 * L.n - 1) Lw <<= 1;
    if (Lw > ((int64_t)1 << 26)) return fail(GFFT_ERR_UNSUPPORTED, "transform length too large for Bluestein");
    int rc = get_bluestein(L.n, Lw, prec, &chirp, &B);
    if (rc) return rc;
  }
  need(pl, BUF_AUX, (size_t)L.outer * Lw * L.inner * esz);
  PointDesc pt{};
  pt.outer = L.outer;
  pt.inner = L.inner;
  pt.n = L.n;
  pt.nin = L.nin;
  pt.nout = L.nout;
  pt.Lw = Lw;
  pt.mode = L.mode;
  pt.chirp = chirp;
  pt.B = B;
  Pass e;
  e.kind = PK_EMBED;
  e.pt = pt;
  // inverse transform = conj . forward . conj: the embed conjugates its input.  With Bluestein the
  // forward machinery runs in between; without it the complex engine does the inverse itself.
  e.pt.conj = (bluestein && L.inverse) ? 1 : 0;
  e.src = L.src;
  e.dst = BUF_AUX;
  e.logical_first = true;
  pl->passes.push_back(e);
  Line C{L.outer, L.inner, Lw, Lw, Lw, MODE_C2C, false, BUF_AUX, BUF_AUX};
  int rc;
  if (bluestein) {
    rc = plan_line(pl, C, false);
    if (rc) return rc;
    Pass m;
    m.kind = PK_MULB;
    m.pt = pt;
    m.src = m.dst = BUF_AUX;
    pl->passes.push_back(m);
    C.inverse = true;
    rc = plan_line(pl, C, false);
    if (rc) return rc;
  } else {
    C.inverse = L.inverse;
    rc = plan_line(pl, C, false);
    if (rc) return rc;
  }
  Pass x;
  x.kind = PK_EXTRACT;
  x.pt = pt;
  x.pt.conj = (bluestein && L.inverse) ? 1 : 0;
  x.extra_scale = bluestein ? 1.0 / (double)Lw : 1.0;
  x.src = BUF_AUX;
  x.dst = L.dst;
  pl->passes.push_back(x);
  return GFFT_OK;
}

// ---- real-to-real kinds (DCT / DST I-IV; FFTW's REDFTxx / RODFTxx, fftw_planxfftn.c:68-75) ------
// Every kind is one complex DFT of its logical length N (2(n-1), 2n or 2(n+1): the figure
// get_normalization uses, xfftn.py:763-806) between two pointwise passes:
//   z[pos0 + j] = pre[j] x[j]  (zeros elsewhere)  ->  Z = DFT_N z  ->  y[k] = Re(post[k] Z[idx0 + k])
// with (theta = pi/(2n))
//   REDFT00  N=2(n-1)  pre = 1,2,...,2,1                         post = 1
//   REDFT10  N=2n      pre = 1                                   post = 2 e^{-i k theta}
//   REDFT01  N=2n      pre = (1,2,2,...) e^{-i j theta}          post = 1
//   REDFT11  N=2n      pre = e^{-i j theta}                      post = 2 e^{-i (2k+1) theta/2}
//   RODFT00  N=2(n+1)  pre = 1, pos0 = 1                         post = 2i, idx0 = 1
//   RODFT10  N=2n      pre = 1                                   post = 2i e^{-i (k+1) theta}, idx0 = 1
//   RODFT01  N=2n      pre = i (2,...,2,1) e^{-i (j+1) theta}, pos0 = 1      post = 1
//   RODFT11  N=2n      pre = e^{-i j theta}                      post = 2i e^{-i (2k+1) theta/2}
// (cos/sin sums written as real parts of complex exponentials).  The complex transform runs on
// whatever plan_line picks for N, so every length works; the cost is that of a length-N complex
// transform per n real samples -- these kinds are a convenience of the API, not its hot path.
std::map<std::tuple<int, int64_t, int, int64_t>, R2RTables> g_r2r_cache;   // (kind, n, precision + device, test-hook signature)

int64_t r2r_logical_n(int kind, int64_t n) {
  if (kind == GFFT_REDFT00) return 2 * (n - 1);
  if (kind == GFFT_RODFT00) return 2 * (n + 1);
  return 2 * n;
}

int get_r2r_tables(int kind, int64_t n, int prec, R2RTables *out) {
  std::lock_guard<std::mutex> lock(g_tw_mutex);
  const int e = opts().debug_r2r_exp;
  const int64_t wrong = e > 0 ? ((int64_t)opts().debug_r2r_index % n + n) % n : -1;
  const bool wrong_post = opts().debug_r2r_post != 0;
  auto key = std::make_tuple(kind, n, dev_prec(prec), e > 0 ? ((wrong * 64 + (e & 63)) * 2 + (wrong_post ? 1 : 0)) + 1 : (int64_t)0);
  auto it = g_r2r_cache.find(key);
  if (it == g_r2r_cache.end()) {
    const long double PI = 3.14159265358979323846264338327950288L;
    const long double th = PI / (2.0L * (long double)n);
    std::vector<long double> ar(n), ai(n), br(n), bi(n);
    auto cis = [](long double a, long double *re, long double *im) { *re = cosl(a); *im = -sinl(a); };   // e^{-ia}
    for (int64_t j = 0; j < n; ++j) {
      long double pr = 1, pi_ = 0, qr = 1, qi = 0, c, sre, sim;
      switch (kind) {
        case GFFT_REDFT00: pr = (j == 0 || j == n - 1) ? 1 : 2; break;
        case GFFT_REDFT10: cis(th * j, &sre, &sim); qr = 2 * sre; qi = 2 * sim; break;
        case GFFT_REDFT01: c = j == 0 ? 1 : 2; cis(th * j, &sre, &sim); pr = c * sre; pi_ = c * sim; break;
        case GFFT_REDFT11:
          cis(th * j, &pr, &pi_);
          cis(th * (2 * j + 1) / 2, &sre, &sim); qr = 2 * sre; qi = 2 * sim; break;
        case GFFT_RODFT00: qr = 0; qi = 2; break;
        case GFFT_RODFT10: cis(th * (j + 1), &sre, &sim); qr = -2 * sim; qi = 2 * sre; break;      // 2i (sre + i sim)
        case GFFT_RODFT01:
          c = j == n - 1 ? 1 : 2; cis(th * (j + 1), &sre, &sim); pr = -c * sim; pi_ = c * sre; break;   // i c (..)
        case GFFT_RODFT11:
          cis(th * j, &pr, &pi_);
          cis(th * (2 * j + 1) / 2, &sre, &sim); qr = -2 * sim; qi = 2 * sre; break;
      }
      ar[j] = pr; ai[j] = pi_; br[j] = qr; bi[j] = qi;
    }
    if (wrong >= 0) (wrong_post ? br : ar)[wrong] += (long double)std::pow(10.0, -e);   // (test hook, Options::debug_r2r_exp)
    auto upload = [&](const std::vector<long double> &xr, const std::vector<long double> &xi, void **dst) -> int {
      std::vector<unsigned char> h(xr.size() * 2 * prec);
      for (size_t j = 0; j < xr.size(); ++j) {
        if (prec == 8) { ((double *)h.data())[2 * j] = (double)xr[j]; ((double *)h.data())[2 * j + 1] = (double)xi[j]; }
        else { ((float *)h.data())[2 * j] = (float)xr[j]; ((float *)h.data())[2 * j + 1] = (float)xi[j]; }
      }
      HIP_TRY(hipMalloc(dst, h.size()));
      HIP_TRY(hipMemcpy(*dst, h.data(), h.size(), hipMemcpyHostToDevice));
      return GFFT_OK;
    };
    R2RTables t{nullptr, nullptr};
    int rc = upload(ar, ai, &t.pre);
    if (rc) return rc;
    rc = upload(br, bi, &t.post);
    if (rc) return rc;
    it = g_r2r_cache.emplace(key, t).first;
  }
  *out = it->second;
  return GFFT_OK;
}

}  // namespace

// one real-to-real axis: [outer][n][inner] real -> same shape; src/dst in {BUF_IN, BUF_OUT}
int plan_r2r_line(gfft_plan_s *pl, int64_t outer, int64_t n, int64_t inner, int kind, int src, int dst) {
  const int prec = pl->precision;
  if (kind == GFFT_REDFT00 && n < 2) return fail(GFFT_ERR_INVALID, "REDFT00 needs at least two points");
  const int64_t N = r2r_logical_n(kind, n);
  R2RTables t;
  int rc = get_r2r_tables(kind, n, prec, &t);
  if (rc) return rc;
  const double lines = (double)outer * (double)inner;
  pl->flops += 2.5 * (double)N * std::log2((double)(N > 1 ? N : 2)) * lines;
  pl->bytes += lines * 2.0 * (double)n * prec;
  if ((pow2_r2r_supported((int)N) || (N <= 4096 && (mix3_supported((int)N) || mix5_supported((int)N)))) &&
      !opts().force_generic && outer * inner < ((int64_t)1 << 31)) {
    // one register-kernel pass: the pointwise steps are load / store adapters of the length-N
    // complex transform (MODE_R2R), so the line is read once and written once
    Pass p;
    p.regk = true;
    p.cols = inner > 1;
    p.logical_first = true;
    p.src = src;
    p.dst = dst;
    PassDesc &d = p.d;
    d.n = (int)N;
    d.mode = MODE_R2R;
    d.batch = outer * inner;
    d.mid = 1;
    d.inner = inner;
    d.in_os = d.out_os = n * inner;
    d.in_is = d.out_is = 1;
    d.in_es = d.out_es = inner;
    d.scale = 1.0;
    d.r2r_pre = t.pre;
    d.r2r_post = t.post;
    d.r2r_n = (int)n;
    d.r2r_pos0 = (kind == GFFT_RODFT00 || kind == GFFT_RODFT01) ? 1 : 0;
    d.r2r_idx0 = (kind == GFFT_RODFT00 || kind == GFFT_RODFT10) ? 1 : 0;
    rc = get_twiddles(N, prec, &d.tw);
    if (rc) return rc;
    pl->passes.push_back(p);
    return GFFT_OK;
  }
  need(pl, BUF_WS, (size_t)outer * N * inner * 2 * prec);
  PointDesc pt{};
  pt.outer = outer;
  pt.inner = inner;
  pt.n = n;
  pt.nin = pt.nout = n;
  pt.Lw = N;
  pt.mode = MODE_R2R;
  pt.pre = t.pre;
  pt.post = t.post;
  pt.pos0 = (kind == GFFT_RODFT00 || kind == GFFT_RODFT01) ? 1 : 0;
  pt.idx0 = (kind == GFFT_RODFT00 || kind == GFFT_RODFT10) ? 1 : 0;
  Pass e;
  e.kind = PK_EMBED;
  e.pt = pt;
  e.src = src;
  e.dst = BUF_WS;
  e.logical_first = true;
  pl->passes.push_back(e);
  Line C{outer, inner, N, N, N, MODE_C2C, false, BUF_WS, BUF_WS};
  rc = plan_line(pl, C, false);
  if (rc) return rc;
  Pass x;
  x.kind = PK_EXTRACT;
  x.pt = pt;
  x.src = BUF_WS;
  x.dst = dst;
  pl->passes.push_back(x);
  return GFFT_OK;
}

static int64_t max_prime_factor(int64_t n) {
  int64_t m = 1;
  for (int64_t p = 2; p * p <= n; ++p)
    while (n % p == 0) { m = p; n /= p; }
  return n > 1 ? n : m;
}

// Build the kernel passes of one transformed axis.
int plan_line(gfft_plan_s *pl, const Line &L, bool top) {
  const int prec = pl->precision;
  const int64_t n = L.n;
  const int64_t batch = L.outer * L.inner;
  if (batch >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
    return fail(GFFT_ERR_UNSUPPORTED, "batch or length exceeds 2^31");
  if (top) {
    const double lines = (double)batch;
    if (n > 1) pl->flops += (L.mode == MODE_C2C ? 1.0 : 0.5) * 5.0 * (double)n * std::log2((double)n) * lines;
    const double esz_in = (L.mode == MODE_R2C) ? prec : 2.0 * prec;
    const double esz_out = (L.mode == MODE_C2R) ? prec : 2.0 * prec;
    pl->bytes += lines * ((double)L.nin * esz_in + (double)L.nout * esz_out);
  }
  Pass p;
  p.d = natural_desc(L);
  p.src = L.src;
  p.dst = L.dst;
  p.logical_first = true;
  const int gmax = generic_max_n(prec);
  if (real_half_ok(L, prec)) {
    // contiguous real lines of even length: one complex transform of HALF the length on the line
    // read / written as complex pairs, Hermitian pass in registers (fft_real_*.hip)
    if (regk_ok(n, prec)) {
      p.has_full = true;
      p.full = p.d;
      int rc = get_twiddles(n, prec, &p.full.tw);
      if (rc) return rc;
    }
    half_desc(&p.d, L);
    p.regk = true;
    p.cols = false;
    int rc = get_twiddles(n / 2, prec, &p.d.tw);
    if (!rc) rc = get_twiddles(n, prec, &p.d.rtw);
    if (rc) return rc;
    pl->passes.push_back(p);
    return GFFT_OK;
  }
  if (regk_ok(n, prec) || regk_c2c_ok(n, prec, L.mode)) {
    p.regk = true;
    p.cols = L.inner > 1;
    int rc = get_twiddles(n, prec, &p.d.tw);
    if (rc) return rc;
    pl->passes.push_back(p);
    return GFFT_OK;
  }
  int64_t n1 = 0, n2 = 0;
  // 2^a 3^b 5^c lengths the single-pass tables miss (960 = 48 x 20, 1920 = 96 x 20, ...): two
  // register-kernel passes (~2.5 TB/s effective) beat the LDS generic kernel (0.5-1.5 TB/s)
  // ... and lengths with one more small prime (896 = 128 x 7, 1792 = 256 x 7, 1408 = 128 x 11):
  // a register-kernel pass plus a tiny generic pass.
  if (L.mode == MODE_C2C && n >= 240 && !opts().force_generic) {
    int64_t both = 0, one = 0;
    // a single prime factor 7 / 11 / 13 beside a register-kernel length: that pass is one column
    // per thread (fft_generic.hip, tiny_dft_kernel) and runs at strided-copy speed
    for (int64_t a : {7, 11, 13})
      if (n % a == 0 && regk_ok(n / a, prec)) one = a;
    for (int64_t a = (int64_t)std::sqrt((double)n); a >= 2; --a) {
      if (n % a) continue;
      const int64_t b = n / a;
      if (a >= 16 && regk_ok(a, prec) && regk_ok(b, prec)) { both = a; break; }
      Factors fa;
      if (!one && a <= 61 && regk_ok(b, prec) && factorize(a, &fa, GENERIC_MAX_PRIME)) one = a;
    }
    if (both) return plan_fourstep(pl, L, n / both, both);
    if (one) return plan_fourstep(pl, L, n / one, one);
  }
  if (n <= gmax && factorize(n, &p.f, GENERIC_MAX_PRIME)) {
    int rc = get_twiddles(n, prec, &p.d.tw);
    if (rc) return rc;
    pl->passes.push_back(p);
    return GFFT_OK;
  }
  if (max_prime_factor(n) <= GENERIC_MAX_PRIME && split_long(n, prec, &n1)) {
    if (L.mode == MODE_C2C) return plan_long(pl, L, n1, n / n1);
    return plan_embedded(pl, L, false);                                       // real: as a complex line of the same length
  }
  const bool splittable = max_prime_factor(n) <= GENERIC_MAX_PRIME && split_fourstep(n, prec, &n1, &n2);
  if (L.mode == MODE_C2C && splittable) return plan_fourstep(pl, L, n1, n2);
  if (L.mode != MODE_C2C && splittable) return plan_embedded(pl, L, false);   // real, long, composite
  return plan_embedded(pl, L, true);                                          // Bluestein
}

// ---- 3-D all-axes plans on one GPU: pass order + padded-pitch workspace --------------------
// Strided passes over power-of-two pitches alias onto few HBM channels (measured on MI355X,
// 1024^3 c128: the axis-0 pass takes 11.0 ms on natural strides, 7.4 ms when rows are pitched
// 256 B wider).  User-visible arrays must stay C-contiguous, so the plan routes the data through
// one internal workspace W whose rows carry that extra pitch, and orders the passes so that each
// user array is touched by the pass that tolerates its layout best:
//   forward / r2c :  axis2 (rows) IN -> W | axis0 (cols) W -> W in place | axis1 (cols) W -> OUT
//   backward / c2r:  axis1 (cols) IN -> W | axis0 (cols) W -> W in place | axis2 (rows) W -> OUT
// Each pass still reads and writes every element exactly once (algorithmic traffic only).
bool fused3_applicable(const gfft_plan_s *pl) {
  if (!opts().fused3 || pl->ndims != 3 || pl->axes.size() != 3) return false;
  const bool real = pl->kind == GFFT_R2C || pl->kind == GFFT_C2R;
  if (real && pl->axes.back() != 2) return false;
  const std::vector<int64_t> &full = (pl->kind == GFFT_C2R) ? pl->sizes_out : pl->sizes_in;
  for (int i = 0; i < 3; ++i)
    if (!regk_ok(full[i], pl->precision) && !(pl->trunc.empty() && ((!real || i < 2) ? regk_c2c_ok(full[i], pl->precision, MODE_C2C)
                                                                                       : (full[i] % 2 == 0 && real_half_mixv_ok(full[i] / 2))))) return false;
  const int64_t bytes = full[0] * full[1] * full[2] * (real ? 1 : 2) * pl->precision;
  return bytes >= opts().fused3_min_bytes;
}

// algorithmic bytes of one pass of the 3-D schedule: one read + one write of its lines (nc_full: complex entries of a
// transformed row); strided passes tile the line-rounded width, the model counts the data columns
static double fused3_pass_bytes(const Pass &p, int prec, int64_t nc_full) {
  const double esz = 2.0 * prec;
  const bool half = p.d.mode == MODE_R2C_H || p.d.mode == MODE_C2R_H;
  const double lines = p.data_inner ? (double)p.d.batch / (double)p.d.inner * (double)p.data_inner : (double)p.d.batch;
  const double n = half ? 2.0 * p.d.n : p.d.n;          // logical length of the line
  const bool r2c = p.d.mode == MODE_R2C || p.d.mode == MODE_R2C_H, c2r = p.d.mode == MODE_C2R || p.d.mode == MODE_C2R_H;
  const double ein = r2c ? prec : esz, eout = c2r ? prec : esz;
  double nin = c2r ? (double)nc_full : n, nout = r2c ? (double)nc_full : n;
  if (p.d.tr_dir == 1) nout = p.d.tr_n;
  if (p.d.tr_dir == 2) nin = p.d.tr_n;
  return lines * (nin * ein + nout * eout);
}

int plan_fused3(gfft_plan_s *pl) {
  const int prec = pl->precision;
  const bool real = pl->kind == GFFT_R2C || pl->kind == GFFT_C2R;
  const bool inverse = pl->kind == GFFT_C2C_BACKWARD || pl->kind == GFFT_C2R;
  // the transformed (padded, physical-side) lengths; with gfft_plan_create_padded the spectral side
  // keeps t0 x t1 x nc entries of them (3/2-rule truncation / zero padding fused into every pass)
  const std::vector<int64_t> &full = inverse ? pl->sizes_out : pl->sizes_in;
  const int64_t n0 = full[0], n1 = full[1], n2 = full[2];
  const bool tr = pl->trunc.size() == 3;
  const int64_t nc_full = real ? n2 / 2 + 1 : n2;      // complex entries per transformed row
  const int64_t nc = tr ? pl->trunc[2] : nc_full;      // complex entries per stored row
  const int64_t t0 = tr ? pl->trunc[0] : n0, t1 = tr ? pl->trunc[1] : n1;
  auto keep = [&](Pass &p, int64_t kept, int64_t of) {   // libfft.py:263-311 as the pass's store / load adapter
    if (kept != of) set_truncation(p.d, inverse ? 2 : 1, kept);
  };
  const int64_t esz = 2 * prec;
  const int64_t seg = 128 / esz;      // (R4: rows in whole 256-byte pieces instead measured +1 % on the real fp64 schedule: more padding columns, nothing gained)
  // columns the in-workspace passes run over: nc rounded up to whole 128-byte lines (the padding
  // columns hold zeros written by the pass that fills W), see PassDesc::inner_ld / inner_st
  const int64_t Pu = (nc + seg - 1) / seg * seg;
  // workspace row pitch: rows start on 128-B lines, under both pitch rules
  const int64_t P = pitch_off_129(pitch_off_2k(Pu, esz), esz);
  need(pl, BUF_WS, (size_t)(n0 * n1 * P * esz));
  pl->ws_pitch = P;

  auto base = [&](int n, int mode) {
    Pass p;
    p.regk = true;
    p.logical_first = true;
    p.d.n = n;
    p.d.mode = mode;
    p.d.conj_in = inverse ? 1 : 0;
    p.d.conj_out = (inverse && mode != MODE_C2R) ? 1 : 0;
    p.d.scale = 1.0;
    p.d.mid = 1;
    p.d.inner = 1;
    p.d.in_ms = p.d.out_ms = 0;
    p.d.in_is = p.d.out_is = 1;
    return p;
  };
  // Workspace layout W[i1][i0][c] (row pitch P): axis 0 is the NEAR strided axis inside W
  // (stride P), axis 1 the far one (stride n0*P).  The in-place middle pass then runs on near
  // strides on both its sides, and the pass that touches the user's natural array does so along
  // axis 1, the near axis of the natural layout (measured: near pad->pad 7.2 ms, far 7.9 ms).
  int64_t w_i0 = P, w_i1 = n0 * P;
  // tile-major workspace (option wtile, decided below once the pair is known): W[i0][tile of TWc columns][k1][TWc], planes w_i0 apart
  bool wtile = false;
  int wt_lg = 0;
  int64_t TWc = 0, wtS = 0;          // columns of a tile; entries from one tile to the next
  // Forward r2c with rows that are not whole lines wide (odd n/2 + 1): the pass that writes the
  // caller's array would store 256-byte segments off the line grid (4.6-5.0 ms per 1024^3 pass
  // against 3.4 aligned).  Stores hurt more than loads (tools/flat_probe.py), so that pass becomes
  // the FAR-axis one with tiles over the flattened (i1, c) index of the output -- aligned stores
  // whenever n1 * (n/2+1) * 16 B is a multiple of 128 -- reading the workspace, now W[i0][i1][c],
  // through per-lane (row, column) addresses (misaligned loads, 3.8 ms).  Backward keeps the
  // layout above: its first pass already has the misalignment on the load side.
  const bool flat_out = real && !inverse && !tr && Pu != nc && (n1 * nc * esz) % 128 == 0 && opts().flat_out;
  if (flat_out) { w_i0 = n1 * P; w_i1 = P; }
  // rows: transform along axis 2.  The batch runs fastest along whichever of (i0, i1) makes the
  // rows it READS consecutive in memory (reading scattered 16-KiB rows measured 6.7 ms per pass,
  // writing them scattered 5.8 ms): forward reads the natural array -> i1 fastest; backward
  // reads W[i1][i0][c] -> i0 fastest.  Strides are in elements of each side's own type.
  auto rows = [&](int mode, bool in_ws, bool out_ws, int src, int dst) {
    Pass p = base((int)n2, mode);
    p.cols = false;
    p.d.batch = n0 * n1;
    const int64_t nat_in = n2, nat_out = n2;   // the natural side of a row pass is the physical array
    const int64_t in_i0 = in_ws ? w_i0 : n1 * nat_in, in_i1 = in_ws ? w_i1 : nat_in;
    const int64_t out_i0 = out_ws ? w_i0 : n1 * nat_out, out_i1 = out_ws ? w_i1 : nat_out;
    if (!in_ws) {   // o = i0, i = i1
      p.d.inner = n1;
      p.d.in_os = in_i0;   p.d.in_is = in_i1;
      p.d.out_os = out_i0; p.d.out_is = out_i1;
    } else {        // o = i1, i = i0
      p.d.inner = n0;
      p.d.in_os = in_i1;   p.d.in_is = in_i0;
      p.d.out_os = out_i1; p.d.out_is = out_i0;
    }
    p.d.in_es = 1;
    p.d.out_es = 1;
    if (wtile && in_ws) { p.d.in_os = TWc; p.d.in_tlg = wt_lg; p.d.in_tS = wtS; }          // (o = k1: one row of a tile; the line itself tile-major)
    if (wtile && out_ws) { p.d.out_os = TWc; p.d.out_tlg = wt_lg; p.d.out_tS = wtS; }
    p.src = src; p.dst = dst;
    if (mode != MODE_C2C && n2 % 2 == 0 &&
        (real_half_supported((int)(n2 / 2)) || real_half_mix_supported((int)(n2 / 2)) || real_half_mixv_ok(n2 / 2))) {
      // packed-real form: complex length n2/2, the real side (the user's natural array) in pairs
      p.d.n = (int)(n2 / 2);
      p.d.mode = mode == MODE_R2C ? MODE_R2C_H : MODE_C2R_H;
      p.d.conj_in = 0;
      p.d.conj_out = mode == MODE_C2R ? 1 : 0;
      if (mode == MODE_R2C) { p.d.in_os /= 2; p.d.in_is /= 2; }
      else { p.d.out_os /= 2; p.d.out_is /= 2; }
      if (mode == MODE_R2C && out_ws) p.d.out_pad = (int)(Pu - nc);
    }
    keep(p, nc, nc_full);
    return p;
  };
  // axis 1: batch (o = i0, i = c)
  auto axis1 = [&](bool in_ws, bool out_ws, int src, int dst) {
    Pass p = base((int)n1, MODE_C2C);
    p.cols = true;
    // tiles cover the line-rounded width; the natural side is masked to its nc columns
    p.d.batch = t0 * Pu;
    p.d.inner = Pu;
    p.data_inner = nc;
    if (Pu != nc) {
      if (!in_ws) p.d.inner_ld = nc;
      if (!out_ws) p.d.inner_st = nc;
    }
    p.d.in_os = in_ws ? w_i0 : t1 * nc;   p.d.in_es = in_ws ? w_i1 : nc;
    p.d.out_os = out_ws ? w_i0 : t1 * nc; p.d.out_es = out_ws ? w_i1 : nc;
    if (wtile && in_ws) { p.d.in_es = TWc; p.d.in_ilg = wt_lg; p.d.in_iS = wtS; }
    if (wtile && out_ws) { p.d.out_es = TWc; p.d.out_ilg = wt_lg; p.d.out_iS = wtS; }      // every tile one contiguous run
    p.src = src; p.dst = dst;
    keep(p, t1, n1);
    return p;
  };
  // axis 0 inside the workspace: batch (o = i1, i = c)
  auto axis0 = [&](int src, int dst) {
    Pass p = base((int)n0, MODE_C2C);
    p.cols = true;
    p.d.batch = n1 * Pu;
    p.d.inner = Pu;
    p.data_inner = nc;
    p.d.in_os = w_i1;  p.d.in_es = w_i0;
    p.d.out_os = w_i1; p.d.out_es = w_i0;
    if (wtile) {          // k1 advances by one row of a tile, the columns are tile-major
      p.d.in_os = p.d.out_os = TWc;
      p.d.in_ilg = p.d.out_ilg = wt_lg;
      p.d.in_iS = p.d.out_iS = wtS;
    }
    p.src = src; p.dst = dst;
    keep(p, t0, n0);      // in place: a column is loaded whole before its first entry is stored
    return p;
  };
  // axis 0 from W[i0][i1][c] to the natural output, tiles over the flattened (i1, c) index
  auto axis0_flat = [&](int src, int dst) {
    Pass p = base((int)n0, MODE_C2C);
    p.cols = true;
    p.d.batch = n1 * nc;
    p.d.mid = n1;
    p.d.inner = nc;
    p.d.flat = 1;
    p.d.in_os = 0;  p.d.in_ms = w_i1;  p.d.in_es = w_i0;
    p.d.out_os = 0; p.d.out_ms = nc;   p.d.out_es = n1 * nc;
    p.src = src; p.dst = dst;
    return p;
  };
  // A complex transform may run its axes in either order.  Where the last two passes can be fused into one
  // launch (make_fused2, FUSED_COLS_ROWS) the forward direction takes the backward schedule's order -- axis 1,
  // then [axis 0 -> rows] plane by plane: the fused pair then WRITES the caller's rows scattered (plane i1 =
  // rows 16 MiB apart), which costs nothing, where the mirror pair [rows -> axis 0] READS them scattered and
  // loses what the fusion gains (1024^3 c128, tools/fused2_probe.py: 20.0 ms against 18.4 ms).
  const bool pair_cols_rows = !real && !tr && !flat_out && Pu == nc && fused2_pair(prec, FUSED_COLS_ROWS, (int)n0, (int)n2, n0 * P * esz, (int)n1).pair;
  // Real transforms: forward [r2c rows -> axis 1] on the contiguous planes i0 of the flat_out schedule (FUSED_R2C_PLANES),
  // backward [axis 0 -> c2r rows] on the planes i1 (FUSED_COLS_C2R), as the complex schedule runs its last two passes
  const bool pair_real = real && !tr && n2 % 2 == 0 &&
                         (inverse ? fused2_pair(prec, FUSED_COLS_C2R, (int)n0, (int)(n2 / 2), n0 * P * esz, (int)n1).pair != nullptr
                                  : flat_out && fused2_pair(prec, FUSED_R2C_PLANES, (int)(n2 / 2), (int)n1, n1 * P * esz, (int)n0).pair);
  if (pair_real && inverse) { w_i0 = n1 * P; w_i1 = P; }     // (as under the complex pair, below)
  const bool cols_first = !inverse && pair_cols_rows;
  // ... and the workspace then is W[i0][k1][c]: the stand-alone axis-1 pass stores on NEAR strides (stores are
  // what far strides hurt), the fused pair's axis-0 tiles read the far (pitched) ones
  if (pair_cols_rows) { w_i0 = n1 * P; w_i1 = P; }
  // Tile-major workspace under that schedule (option wtile): the stand-alone axis-1 pass then WRITES every tile of 256-byte segments
  // as one contiguous 256 KiB run -- measured on the pass alone, same buffers (tools/tile_major_probe.py): 6.48 -> 5.84 ms at 1024^3
  // complex128, reading such a buffer is level -- and the pair's strided tiles read W[i0][tile][k1][.] one 256-byte row per plane.
  // In the whole schedule, same arrays (profiles/r05_ab_wtile.txt): 1024^3 c128 31.7 -> 31.0 ms per step (the pass 6.15 -> 5.85 ms,
  // the pair level), (1024,512,1024) -2.0 %, 512^3 -0.9 %, 1024^3 c64 -0.5 %; 960^3 -0.4 %, 896^3 +1.0 %, (1024,2048,1024) +0.4 %:
  // taken where axis 1 is a power of two up to 1024 (option wtile = 2: wherever the layout fits).
  const bool wtile_len = (n1 & (n1 - 1)) == 0 && n1 <= 1024;
  // (The UNFUSED complex schedules on this layout: the pass that fills W gains as much -- 768^3 c128 3.40 -> 3.15 ms, 1152^3 c64
  // 6.60 -> 5.59 -- and the in-place pass, now on the far stride, loses more -- 2.94 -> 3.51, 5.94 -> 6.35: +2.7 % / -1.4 % per step,
  // profiles/r05_ab_wtile.txt part 4; they keep W[i1][i0][c].)
  // The stand-alone forms of a voided pair read the rows tile-major: their thread layout has to advance by whole tiles.
  const bool wtile_rows = pow2_rows_nt(n2, prec) > 0 && pow2_rows_nt(n2, prec) % (int)(256 / esz) == 0 && is_pow2(n0);
  if (pair_cols_rows && opts().wtile && wtile_rows && (wtile_len || opts().wtile >= 2) && Pu % (256 / esz) == 0) {
    wtile = true;
    TWc = 256 / esz;
    pl->ws_tile = (int)TWc;
    while (((int64_t)1 << wt_lg) < TWc) ++wt_lg;
    wtS = n1 * TWc;          // (rows of padding after every tile -- 1, 3, 8 -- measured level: profiles/r05_ab_wtile.txt)
  }
  std::vector<Pass> seq;
  if (flat_out) {
    seq.push_back(rows(MODE_R2C, false, true, BUF_IN, BUF_WS));
    seq.push_back(axis1(true, true, BUF_WS, BUF_WS));
    seq.push_back(axis0_flat(BUF_WS, BUF_OUT));
  } else if (!inverse && !cols_first) {
    seq.push_back(rows(real ? MODE_R2C : MODE_C2C, false, true, BUF_IN, BUF_WS));
    seq.push_back(axis0(BUF_WS, BUF_WS));
    seq.push_back(axis1(true, false, BUF_WS, BUF_OUT));
  } else {
    seq.push_back(axis1(false, true, BUF_IN, BUF_WS));
    seq.push_back(axis0(BUF_WS, BUF_WS));
    seq.push_back(rows(real ? MODE_C2R : MODE_C2C, true, false, BUF_WS, BUF_OUT));
  }
  for (Pass &p : seq) {
    int rc = get_twiddles(p.d.n, prec, &p.d.tw);
    if (rc) return rc;
    const bool half = p.d.mode == MODE_R2C_H || p.d.mode == MODE_C2R_H;
    if (half && (rc = get_twiddles(2 * (int64_t)p.d.n, prec, &p.d.rtw))) return rc;
    // (strided passes tile the line-rounded width Pu; the work model counts the nc data columns)
    const double lines = p.data_inner ? (double)p.d.batch / (double)p.d.inner * (double)p.data_inner : (double)p.d.batch;
    const double n = half ? 2.0 * p.d.n : p.d.n;          // logical length of the line
    pl->flops += (p.d.mode == MODE_C2C ? 1.0 : 0.5) * 5.0 * n * std::log2(n) * lines;
    pl->bytes += fused3_pass_bytes(p, prec, nc_full);
    pl->passes.push_back(p);
  }
  // passes[i], passes[i + 1] as one launch where the pair exists: dA / dB = the two passes on one plane (make_fused2)
  auto fuse = [&](size_t i, int kind, const PassDesc &dA, const PassDesc &dB, int64_t planes, int64_t a_in_plane, int64_t b_out_plane, int64_t slot_bytes) {
    Pass f;
    if (!make_fused2(pl, kind, pl->passes[i], pl->passes[i + 1], dA, dB, (int)planes, a_in_plane, b_out_plane, slot_bytes, &f)) return;
    f.bytes2 = fused3_pass_bytes(pl->passes[i], prec, nc_full) + fused3_pass_bytes(pl->passes[i + 1], prec, nc_full);
    pl->passes[i] = f;
    pl->passes.erase(pl->passes.begin() + i + 1);
  };
  // Complex schedules: [rows along axis 2] + [axis 0 inside the workspace] -- passes 1 + 2 forward, 2 + 3
  // backward -- as ONE persistent launch per direction, plane by plane (a plane = one i1: n0 rows of n2
  // entries), the plane handed over through the Infinity Cache instead of W (FUSED_ROWS_COLS / _COLS_ROWS).
  if (!real && !tr && !flat_out && Pu == nc && pl->passes.size() >= 3) {
    const size_t base = pl->passes.size() - 3;
    const Pass &p1 = pl->passes[base], &p2 = pl->passes[base + 1], &p3 = pl->passes[base + 2];
    if (!inverse && !cols_first) {
      PassDesc dA = p1.d, dB = p2.d;                  // rows IN -> slot[i0][c];  axis 0: slot -> W[i1][k0][c]
      dA.batch = n0; dA.inner = 1; dA.in_is = 0; dA.out_is = 0; dA.out_os = P;
      dB.batch = Pu; dB.in_os = 0; dB.out_os = 0; dB.in_es = P;
      fuse(base, FUSED_ROWS_COLS, dA, dB, n1, n2 * esz, w_i1 * esz, n0 * P * esz);
    } else {
      PassDesc dA = p2.d, dB = p3.d;                  // axis 0: W[i1][k0][c] -> slot[i0][c];  rows slot -> OUT
      dA.batch = Pu; dA.in_os = 0; dA.out_os = 0; dA.out_es = P;
      dB.batch = n0; dB.inner = 1; dB.in_is = 0; dB.out_is = 0; dB.in_os = P; dB.out_os = n1 * n2;
      int64_t a_plane = w_i1 * esz;
      if (wtile) {
        // the pair's kernels take natural-layout descriptors only (PF_NATURAL): the tile-major columns as (tile, column in tile)
        dA.mid = Pu / TWc; dA.inner = TWc;
        dA.in_ms = wtS; dA.in_is = 1; dA.in_ilg = 0; dA.in_iS = 0;
        dA.out_ms = TWc;     dA.out_is = 1; dA.out_ilg = 0; dA.out_iS = 0;
        dB.in_tlg = 0; dB.in_tS = 0;                   // (B reads the slot, natural rows)
        a_plane = TWc * esz;                           // plane k1 = one row of every tile
      }
      fuse(base + 1, FUSED_COLS_ROWS, dA, dB, n1, a_plane, n2 * esz, n0 * P * esz);
    }
  }
  if (pair_real && pl->passes.size() >= 3) {
    const size_t base = pl->passes.size() - 3;
    if (!inverse) {
      const Pass &p1 = pl->passes[base], &p2 = pl->passes[base + 1];
      if (p1.d.mode == MODE_R2C_H && p2.cols) {
        PassDesc dA = p1.d, dB = p2.d;                // r2c rows of plane i0: IN -> slot[i1][c];  axis 1: slot -> W[i0][k1][c]
        dA.batch = n1; dA.inner = 1; dA.in_os = n2 / 2; dA.in_is = 0; dA.out_os = P; dA.out_is = 0;
        dB.batch = Pu; dB.in_os = 0; dB.out_os = 0; dB.in_es = P;
        fuse(base, FUSED_R2C_PLANES, dA, dB, n0, n1 * n2 * prec, w_i0 * esz, n1 * P * esz);
      }
    } else {
      const Pass &p2 = pl->passes[base + 1], &p3 = pl->passes[base + 2];
      if (p3.d.mode == MODE_C2R_H && p2.cols) {
        PassDesc dA = p2.d, dB = p3.d;                // axis 0 of plane i1: W -> slot[i0][c];  c2r rows: slot -> OUT
        dA.batch = Pu; dA.in_os = 0; dA.out_os = 0; dA.out_es = P;
        dB.batch = n0; dB.inner = 1; dB.in_is = 0; dB.out_is = 0; dB.in_os = P; dB.out_os = n1 * n2 / 2;
        fuse(base + 1, FUSED_COLS_C2R, dA, dB, n1, w_i1 * esz, n2 * prec, n0 * P * esz);
      }
    }
  }
  pl->fused3 = true;
  // fp32 strided passes of this schedule run between pitched rows, where two 512-thread workgroups
  // per CU on 128-byte segments (variant 2 of the n = 512 / 1024 tables: one computes while the other
  // loads) beat one 1024-thread workgroup on 256-byte segments since the 4-byte LDS bank rule --
  // whole transforms, tools/variant2_pfft_probe.py: 1024^3 r2c f32 5.78 / 5.87 -> 5.44 / 5.59 ms,
  // 512^3 c64 1.39 / 1.35 -> 1.30 / 1.30 ms, 1024^3 c64 10.7 / 10.9 -> 10.6 / 11.0 ms.  (On natural
  // power-of-two strides -- the stage arrays of multi-GPU transforms -- the wide tile stays ahead.)
  if (prec == GFFT_F32 && pl->variant_cols == 0) pl->variant_cols = 2;
  // fp64 REAL schedules keep the strided kernels of rounds 1-3 (table variant 17: 16 / 8 values per thread, two
  // exchanges): the round-4 defaults -- 32 values per thread, one exchange, non-temporal streams -- gain on complex
  // schedules (1024^3 c128 per step 32.85 -> 32.51 ms) and on natural-stride stage arrays, and lose 1.5-3 % here
  // (1024^3 r2c f64 per step 18.76 -> 19.03 / 19.31 ms, profiles/r04_real_pairs.txt)
  if (prec == GFFT_F64 && real && pl->variant_cols == 0) pl->variant_cols = 17;
  // ... and complex fp64 schedules the round-4 tiles of 16 columns (table variant 16): the 32-column tiles that win 5-12 % on natural-stride
  // arrays since round 6 (n = 256, n = 512 near strides, fft_pow2_f64.hip) LOSE inside this schedule -- its workspace is laid out in
  // 16-column tiles and pitched rows --: 512^3 c128 per step 4.159 -> 4.269 ms, 256^3 0.582 -> 0.600 ms (profiles/r06_cols_t32_probe.txt)
  if (prec == GFFT_F64 && !real && pl->variant_cols == 0) pl->variant_cols = 16;
  // XCD-contiguous tile order for the stand-alone passes of power-of-two schedules (each XCD walks its own eighth of the
  // tiles: neighbouring column chunks of the pitched workspace rows share an L2).  Neutral with the kernels of rounds 1-3
  // (+-0.2 %); with the 512- / 256-thread kernels of round 4, same arrays, plans alternating (profiles/r04_ab_swizzle.txt):
  // 1024^3 c128 per step 30.76 -> 30.52 ms and 32.23 -> 31.50 ms on two boxes (the pass 5.83 -> 5.69 ms), 1024^3 c64 19.42 ->
  // 19.00, 512^3 c128 4.17 -> 4.07, 1024^3 r2c f64 18.65 -> 18.48; level for real fp32 and 512^3 c64, +0.8 % at 768^3
  // (3^b 2^k kernels: left on automatic).  On natural-stride stage arrays (C4 on 8 GPUs) it LOSES 2-8 %: only here.
  if (pl->xcd_swizzle < 0 && is_pow2(n0) && is_pow2(n1) && is_pow2(n2) && !(real && prec == GFFT_F32)) pl->xcd_swizzle = 1;
  // The order IN TIME of that walk (PassDesc::order, option tile_order): complex fp64 power-of-two schedules may take one
  // (their stand-alone pass at n = 1024 has the kernel for it, fft_pow2_f64.hip); 0 = the plain order.  Measured at 1024^3
  // (tools/tile_order_probe.py, profiles/r08_tile_order_probe.txt: orders alternating on the same arrays, ten array sets, both
  // directions): the tiles an XCD runs together taken from TWO planes three planes apart instead of one -- the pass 5.99 -> 5.74 ms
  // forward, 5.92 -> 5.72 ms backward, better on every array set (-0.16 ... -0.26 ms); 37 / 63 / 127 planes apart -0.13 ... -0.22,
  // neighbouring planes -0.05, four or eight planes level or worse.  XCD start offsets and rotated row orders: level or worse
  // (+-0.03, +0.04 ... +0.13 ms).  The kernel's ACCESS PATTERN ALONE loses under the same order (+0.13 ms): the gain is not in
  // the placement of the requests.  Only that shape was measured: only it takes the order by default.
  if (prec == GFFT_F64 && !real && !tr && is_pow2(n0) && is_pow2(n1) && is_pow2(n2))
    pl->tile_order = (n0 == 1024 && n1 == 1024 && n2 == 1024) ? ((1 << ORD_PLANES_LOG2) | (3 << ORD_PLANES_APART)) : 0;      // (two planes together, 3 apart)
  // Workgroups per launch.  Each walks tiles block, block + grid, ...; more, shorter walks balance the
  // tail better, too many lose the overlap of one tile's stores with the next one's loads.  Clean A/B
  // on fixed caller arrays (tools/ab_option_probe.py grid_cap ...), fwd + bwd per step: 1024^3 c128
  // 38.04 (4096) / 37.64 (16384) / 37.50 (32768) / 39.23 ms (65536 = one tile each); 512^3 c128 4.90 /
  // 4.81 / 4.79; 768^3 c128 16.96 / 16.82 / 17.26; 1024^3 c64 20.76 / 20.50 / 20.65 -- but real
  // transforms the other way (1024^3 r2c f64 20.60 / 20.70 / 21.21, f32 11.23 / 11.79): complex
  // schedules take 16384, real ones 8192 (1024^3 r2c f64 20.60 -> 20.48, f32 11.09 -> 11.04 ms; 2048 and
  // 1024 lose 1-2 % each), stand-alone strided passes keep 4096 (GFFT_GRID_CAP overrides them all).
  if (opts().grid_cap <= 0)
    for (Pass &p : pl->passes) p.d.grid_cap = real ? 8192 : ((is_pow2(n0) && is_pow2(n1) && is_pow2(n2)) ? 32768 : 16384);     // (R4, XCD-contiguous order, 32-value kernels: 1024^3 c128 per step 32.23 (4096) / 31.97 (16384) / 31.81 (32768) / 32.07 ms (65536))
  return GFFT_OK;
}

hipError_t run_pass(const gfft_plan_s *pl, const Pass &p, const PassDesc &d0, const void *in, void *out,
                    double scale, hipStream_t s) {
  if (p.kind == PK_EMBED) return launch_embed(p.pt, pl->precision, in, out, s);
  if (p.kind == PK_MULB) return launch_mulb(p.pt, pl->precision, out, s);
  if (p.kind == PK_EXTRACT) return launch_extract(p.pt, pl->precision, in, out, scale * p.extra_scale, s);
  PassDesc d = d0;
  // auto: only where a strided pass WRITES rows that do not start on 128-byte lines (odd-width
  // half spectra): neighbouring chunks then meet in one L2 and their partial lines merge.  For a
  // pass that only READS such rows the order lowers FETCH_SIZE (1.44 -> 1.13 x the algorithmic
  // bytes) but not the time (3.48 ms plain, 3.65 ms XCD-contiguous, tools/flat_probe.py): off.
  // (measured 1024^3 r2c: 5.4 -> 5.0 ms fp64, 3.6 -> 2.6 ms fp32; neutral-to-slightly-negative on
  // aligned arrays, so it stays off there)
  const int64_t esz_out = ((d.mode == MODE_C2R || d.mode == MODE_R2R) ? 1 : 2) * (int64_t)pl->precision;
  const int64_t esz_in = ((d.mode == MODE_R2C || d.mode == MODE_R2R) ? 1 : 2) * (int64_t)pl->precision;
  (void)esz_in;
  // workgroups per launch of stand-alone row passes (the first / last stage of every multi-GPU
  // transform): tools/ab_gridcap_serial.py, caps alternated on one plan and the same arrays --
  // (256,512,1024) c128 rows 0.803 (4096) -> 0.782 ms (16384), (512,1024,2048) f32 r2c rows 1.854 ->
  // 1.803 ms; strided stand-alone passes are level or lose (far axis 1.001 -> 1.037 ms) and keep 4096
  if (!d.grid_cap && p.regk && !p.cols && !pl->fused3 && opts().grid_cap <= 0) d.grid_cap = 16384;
  // ... and of strided passes that READ on a far power-of-two stride (the caller's natural array along its outermost axis: the far
  // stage of every backward distributed transform): more, shorter walks -- (1024,256,512) complex128 natural -> natural 0.895 ->
  // 0.849 ms, natural -> pitched 0.903 -> 0.857 ms; pitched inputs and near axes are level or lose (tools/bwd_probe.py,
  // profiles/r06_bwd_probe.txt)
  if (!d.grid_cap && p.regk && p.cols && !pl->fused3 && opts().grid_cap <= 0 && d.mid == 1 && !d.flat && !d.in_lgp &&
      d.in_es >= ((int64_t)1 << 16) && (d.in_es & (d.in_es - 1)) == 0) d.grid_cap = 16384;
  d.swizzle = pl->xcd_swizzle >= 0 ? pl->xcd_swizzle : (p.cols && !d.flat && ((d.out_es * esz_out) % 128 != 0) ? 1 : 0);
  // (the order in time of that walk: the plan's own, or option tile_order -- read here, at launch time, so that one plan runs both forms)
  d.order = (pl->tile_order >= 0 && p.regk && p.cols && d.swizzle) ? (opts().tile_order >= 0 ? opts().tile_order : pl->tile_order) : 0;
  if ((d.mode == MODE_R2C_H || d.mode == MODE_C2R_H) && real_half_supported(d.n))
    return pl->precision == 8 ? launch_real_half_f64(d, pl->variant_rows, in, out, s)
                              : launch_real_half_f32(d, pl->variant_rows, in, out, s);
  if ((d.mode == MODE_R2C_H || d.mode == MODE_C2R_H) && mixv_supported(d.n))
    return pl->precision == 8 ? launch_real_half_mixv_f64(d, in, out, s) : launch_real_half_mixv_f32(d, in, out, s);
  if (d.mode == MODE_R2C_H || d.mode == MODE_C2R_H)
    return pl->precision == 8 ? launch_real_half_mix_f64(d, in, out, s) : launch_real_half_mix_f32(d, in, out, s);
  if (p.regk && d.mode == MODE_R2R && pow2_r2r_supported(d.n))
    return pl->precision == 8 ? launch_pow2_r2r_f64(d, p.cols, in, out, s) : launch_pow2_r2r_f32(d, p.cols, in, out, s);
  if (p.regk && mix3_supported(d.n)) {
    return pl->precision == 8 ? launch_mix3_f64(d, p.cols, in, out, s) : launch_mix3_f32(d, p.cols, in, out, s);
  }
  if (p.regk && mix5_supported(d.n)) {
    return pl->precision == 8 ? launch_mix5_f64(d, p.cols, in, out, s) : launch_mix5_f32(d, p.cols, in, out, s);
  }
  if (p.regk && mixv_supported(d.n)) {
    return pl->precision == 8 ? launch_mixv_f64(d, p.cols, pl->mixv_variant, in, out, s) : launch_mixv_f32(d, p.cols, pl->mixv_variant, in, out, s);
  }
  if (p.regk) {
    const int variant = p.cols ? pl->variant_cols : pl->variant_rows;
    return pl->precision == 8 ? launch_pow2_f64(d, p.cols, variant, in, out, s)
                              : launch_pow2_f32(d, p.cols, variant, in, out, s);
  }
  return launch_generic(d, p.f, pl->precision, in, out, s);
}

int pow2_grid_cap() { return opts().grid_cap > 0 ? opts().grid_cap : 4096; }
int grid_cap_option() { return opts().grid_cap > 0 ? opts().grid_cap : 0; }
LaunchNote &last_launch() {
  static thread_local LaunchNote note;
  return note;
}

// Batched 2-D complex transform plane by plane: the passes of gfft_plan_create_guru2 (see there), pushed onto pl->passes
// -- one fused launch where a pair exists, else (unless fused_only) the two stand-alone passes [first: IN -> OUT, second:
// in place on OUT].
int build_pair2d(gfft_plan_s *pl, const gfft_iodim *cols, int64_t n2, const gfft_iodim *planes, bool inverse, int cols_first,
                 int in_blocks, int64_t in_block_stride, int out_blocks, int64_t out_block_stride, bool fused_only, bool *fused_out) {
  const int precision = pl->precision;
  const int64_t esz = 2 * (int64_t)precision;
  const int64_t n1 = cols->n, np = planes->n;
  // one side of the array pair as the two passes see it: the strided pass steps es along the axis and jumps between
  // blocks; the row pass places row r = (block m, row i of the block) by its batch strides
  struct Side { int nb; int64_t per, es, bstride, plane; };
  const Side si{in_blocks, n1 / in_blocks, cols->is, in_blocks > 1 ? in_block_stride : (n1 / in_blocks) * cols->is, planes->is};
  const Side so{out_blocks, n1 / out_blocks, cols->os, out_blocks > 1 ? out_block_stride : (n1 / out_blocks) * cols->os, planes->os};

  auto base = [&](int64_t n, bool strided) {
    Pass p;
    p.regk = true;
    p.cols = strided;
    p.logical_first = true;
    p.d.n = (int)n;
    p.d.mode = MODE_C2C;
    p.d.conj_in = p.d.conj_out = inverse ? 1 : 0;
    p.d.mid = 1;
    p.d.inner = 1;
    p.d.in_is = p.d.out_is = 1;
    p.d.in_es = p.d.out_es = 1;
    p.d.scale = 1.0;
    return p;
  };
  auto cols_in = [&](Pass &p, const Side &s) {
    p.d.in_os = s.plane;  p.d.in_es = s.es;
    if (s.nb > 1) { p.d.in_lgp = ilog2_ceil(s.nb);  p.d.in_jump = s.bstride - s.per * s.es; }
    p.blocks[0] = s.nb;  p.bstride[0] = s.nb > 1 ? s.bstride : 0;
  };
  auto cols_out = [&](Pass &p, const Side &s) {
    p.d.out_os = s.plane;  p.d.out_es = s.es;
    if (s.nb > 1) { p.d.out_lgp = ilog2_ceil(s.nb);  p.d.out_jump = s.bstride - s.per * s.es; }
    p.blocks[1] = s.nb;  p.bstride[1] = s.nb > 1 ? s.bstride : 0;
  };
  // the stand-alone forms: the first pass carries the data across (IN -> OUT), the second runs in place on OUT
  Pass pr = base(n2, false), pc = base(n1, true);
  pc.d.batch = np * n2;
  pc.d.inner = n2;
  pr.d.batch = np * n1;
  const Side &rs = (si.nb > 1 && !cols_first) ? si : so;        // the blocks the row pass walks its rows by
  pr.d.mid = rs.nb;  pr.d.inner = rs.per;
  if (!cols_first) {
    pr.d.in_os = si.plane;   pr.d.in_ms = si.nb > 1 ? si.bstride : rs.per * si.es;  pr.d.in_is = si.es;
    pr.d.out_os = so.plane;  pr.d.out_ms = so.nb > 1 ? so.bstride : rs.per * so.es;  pr.d.out_is = so.es;
    pr.src = BUF_IN;  pr.dst = BUF_OUT;
    cols_in(pc, so);  cols_out(pc, so);
    pc.src = BUF_OUT;  pc.dst = BUF_OUT;
  } else {
    cols_in(pc, si);  cols_out(pc, so);
    pc.src = BUF_IN;  pc.dst = BUF_OUT;
    pr.d.in_os = pr.d.out_os = so.plane;
    pr.d.in_ms = pr.d.out_ms = so.bstride;
    pr.d.in_is = pr.d.out_is = so.es;
    pr.src = BUF_OUT;  pr.dst = BUF_OUT;
  }
  int rc = get_twiddles(n2, precision, &pr.d.tw);
  if (!rc) rc = get_twiddles(n1, precision, &pc.d.tw);
  if (rc) return rc;
  // ... and as ONE persistent launch, plane by plane through the Infinity Cache: slot[row of the plane][P]
  bool fused = false;
  if (np < ((int64_t)1 << 30)) {
    const int64_t P = pitch_off_2k(n2, esz);              // slot rows pitched off the power of two
    PassDesc dA, dB;
    Pass f;
    if (!cols_first) {
      dA = pr.d;  dB = pc.d;
      dA.batch = n1;  dA.in_os = 0;  dA.out_os = 0;  dA.out_ms = rs.per * P;  dA.out_is = P;
      dB.batch = n2;  dB.in_os = 0;  dB.out_os = 0;  dB.in_es = P;  dB.in_lgp = 0;  dB.in_jump = 0;
      fused = make_fused2(pl, so.nb > 1 ? FUSED_PLANES_2D_B : FUSED_PLANES_2D, pr, pc, dA, dB, (int)np, si.plane * esz, so.plane * esz, n1 * P * esz, &f);
    } else {
      dA = pc.d;  dB = pr.d;
      dA.batch = n2;  dA.in_os = 0;  dA.out_os = 0;  dA.out_es = P;  dA.out_lgp = 0;  dA.out_jump = 0;
      dB.batch = n1;  dB.in_os = 0;  dB.out_os = 0;  dB.in_ms = rs.per * P;  dB.in_is = P;
      fused = make_fused2(pl, si.nb > 1 ? FUSED_PLANES_CR_B : FUSED_COLS_ROWS, pc, pr, dA, dB, (int)np, si.plane * esz, so.plane * esz, n1 * P * esz, &f);
    }
    if (fused) pl->passes.push_back(f);
  }
  if (!fused && !fused_only) {
    if (!cols_first) { pl->passes.push_back(pr); pl->passes.push_back(pc); }
    else { pl->passes.push_back(pc); pl->passes.push_back(pr); }
  }
  *fused_out = fused;
  return GFFT_OK;
}

// The same for REAL planes (gfft_plan_create_guru2_real, see there): forward [packed-real r2c rows -> strided], backward
// [strided -> packed-real c2r rows], the strided pass addressing the blocks of the half-spectrum side.  `cx` is the
// half-spectrum side (strides in complex entries), `re` the real side (strides in reals, even: the rows are read / written
// as complex pairs); nb / bstride: the blocks of the strided axis on the half-spectrum side.
int build_pair2d_real(gfft_plan_s *pl, int64_t n1, int64_t n2, int64_t np, int64_t re_es, int64_t re_plane, int64_t cx_es,
                      int64_t cx_plane, int nb, int64_t bstride, bool inverse) {
  const int prec = pl->precision;
  const int64_t esz = 2 * (int64_t)prec, m = n2 / 2, H = m + 1, per = n1 / nb;
  // the hand-off slot (and the workspace of the stand-alone backward form): rows of H entries rounded up to whole 128-byte
  // lines, pitched off multiples of 2 KiB and off 129 x 2^k entries (pitch_off_129)
  const int64_t seg = 128 / esz, Pu = (H + seg - 1) / seg * seg;
  const int64_t P = pitch_off_129(Pu, esz);
  // rows: packed-real, complex length m, the real side in pairs
  Pass pr;
  pr.regk = true;
  pr.logical_first = true;
  pr.d.n = (int)m;
  pr.d.mode = inverse ? MODE_C2R_H : MODE_R2C_H;
  pr.d.conj_in = 0;
  pr.d.conj_out = inverse ? 1 : 0;
  pr.d.in_es = pr.d.out_es = 1;
  pr.d.scale = 1.0;
  // strided: complex length n1 along the H columns of a plane; the last tile of columns is masked by `inner` itself (the fused
  // kernels drop inner_ld / inner_st, PF_NATURAL), so nothing is read or written beyond column H - 1 on either side
  Pass pc;
  pc.regk = true;
  pc.cols = true;
  pc.logical_first = true;
  pc.d.n = (int)n1;
  pc.d.mode = MODE_C2C;
  pc.d.conj_in = pc.d.conj_out = inverse ? 1 : 0;
  pc.d.batch = np * H;
  pc.d.mid = 1;
  pc.d.inner = H;
  pc.d.in_is = pc.d.out_is = 1;
  pc.d.scale = 1.0;
  const int lgp = nb > 1 ? ilog2_ceil(nb) : 0;
  const int64_t jump = nb > 1 ? bstride - per * cx_es : 0;
  if (!inverse) {
    // IN (real) -> OUT: row r of plane o = (block r / per, row r % per of the block) placed by the block stride
    pr.d.batch = np * n1;  pr.d.mid = nb;  pr.d.inner = per;
    pr.d.in_os = re_plane / 2;  pr.d.in_ms = per * re_es / 2;  pr.d.in_is = re_es / 2;
    pr.d.out_os = cx_plane;  pr.d.out_ms = nb > 1 ? bstride : per * cx_es;  pr.d.out_is = cx_es;
    pr.src = BUF_IN;  pr.dst = BUF_OUT;
    // ... then the strided pass in place on OUT
    pc.d.in_os = pc.d.out_os = cx_plane;
    pc.d.in_es = pc.d.out_es = cx_es;
    pc.d.in_lgp = pc.d.out_lgp = lgp;  pc.d.in_jump = pc.d.out_jump = jump;
    pc.blocks[0] = pc.blocks[1] = nb;  pc.bstride[0] = pc.bstride[1] = nb > 1 ? bstride : 0;
    pc.src = BUF_OUT;  pc.dst = BUF_OUT;
  } else {
    // strided IN -> WS[plane][row][P] (the caller's input is preserved, and OUT -- real -- is smaller than the half spectrum)
    pc.d.in_os = cx_plane;  pc.d.in_es = cx_es;  pc.d.in_lgp = lgp;  pc.d.in_jump = jump;
    pc.d.out_os = n1 * P;  pc.d.out_es = P;
    pc.blocks[0] = nb;  pc.bstride[0] = nb > 1 ? bstride : 0;
    pc.src = BUF_IN;  pc.dst = BUF_WS;
    // ... then the c2r rows WS -> OUT (real)
    pr.d.batch = np * n1;  pr.d.mid = 1;  pr.d.inner = n1;
    pr.d.in_os = n1 * P;  pr.d.in_is = P;
    pr.d.out_os = re_plane / 2;  pr.d.out_is = re_es / 2;
    pr.src = BUF_WS;  pr.dst = BUF_OUT;
  }
  int rc = get_twiddles(m, prec, &pr.d.tw);
  if (!rc) rc = get_twiddles(2 * m, prec, &pr.d.rtw);
  if (!rc) rc = get_twiddles(n1, prec, &pc.d.tw);
  if (rc) return rc;
  // work model (plan_fused3's): half the flops of a complex line on the real axis, one read + one write per pass
  pl->flops = 0.5 * 5.0 * (double)n2 * std::log2((double)n2) * (double)(np * n1) + 5.0 * (double)n1 * std::log2((double)n1) * (double)(np * H);
  pl->bytes = (double)(np * n1) * ((double)n2 * prec + (double)H * esz) + (double)(np * H) * 2.0 * (double)n1 * esz;
  // ... as ONE persistent launch, plane by plane through the Infinity Cache: slot[row of the plane][P]
  bool fused = false;
  if (np < ((int64_t)1 << 30)) {
    Pass f;
    if (!inverse) {
      PassDesc dA = pr.d, dB = pc.d;      // r2c rows of one plane: IN -> slot (the row's last line completed with zeros); strided: slot -> blocks
      dA.batch = n1;  dA.mid = 1;  dA.inner = 1;  dA.in_os = re_es / 2;  dA.in_ms = 0;  dA.in_is = 0;
      dA.out_os = P;  dA.out_ms = 0;  dA.out_is = 0;  dA.out_pad = (int)(Pu - H);
      dB.batch = H;  dB.in_os = 0;  dB.out_os = 0;  dB.in_es = P;  dB.in_lgp = 0;  dB.in_jump = 0;
      fused = make_fused2(pl, FUSED_R2C_PLANES_B, pr, pc, dA, dB, (int)np, re_plane * prec, cx_plane * esz, n1 * P * esz, &f);
    } else {
      PassDesc dA = pc.d, dB = pr.d;      // strided: blocks -> slot;  c2r rows of one plane: slot -> OUT
      dA.batch = H;  dA.in_os = 0;  dA.out_os = 0;  dA.out_es = P;
      dB.batch = n1;  dB.inner = 1;  dB.in_os = P;  dB.in_is = 0;  dB.out_os = re_es / 2;  dB.out_is = 0;
      fused = make_fused2(pl, FUSED_COLS_C2R_B, pc, pr, dA, dB, (int)np, cx_plane * esz, re_plane * prec, n1 * P * esz, &f);
      if (fused) f.alt_bytes = (size_t)(np * n1 * P * esz);     // (the workspace only the stand-alone form needs)
    }
    if (fused) {
      f.bytes2 = pl->bytes;
      pl->passes.push_back(f);
    }
  }
  if (!fused) {
    if (inverse) need(pl, BUF_WS, (size_t)(np * n1 * P * esz));
    if (!inverse) { pl->passes.push_back(pr); pl->passes.push_back(pc); }
    else { pl->passes.push_back(pc); pl->passes.push_back(pr); }
  }
  pl->passes.back().carries_scale = true;
  return GFFT_OK;
}

}  // namespace gfft
