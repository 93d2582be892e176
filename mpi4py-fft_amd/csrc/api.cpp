// libgfft.so: the C ABI of include/gfft.h (the pseudo-spectral entry points live next to their kernels in spectral.hip, the
// exchange ones in exchange.cpp).  Every entry point checks its arguments first -- a bad call is refused without a device --,
// then looks for the device (check_device) and calls into the planner (plan.cpp, through plan_internal.h).  The codes matter as
// much as the texts: the Python side turns GFFT_ERR_UNSUPPORTED from a creator or a gfft_plan_set_* into "use the slower path"
// and raises on everything else.  The calling thread's error text lives in plan.cpp, with gfft_last_error(), behind fail().
#include "plan_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

using namespace gfft;

namespace {

// ---- options: one table -- the key of gfft_set_option, the environment variable read when the options are first used (most
// have none), and where the value lives: a field of Options (plan_internal.h documents them) or a global of a kernel file.
// "fused3_min_mib" is the one key that is not an int stored as given: gfft_set_option converts it itself.
struct OptionRow { const char *key, *env; int Options::*field; int *global; };
constexpr OptionRow kOptions[] = {
  {"grid_cap", "GFFT_GRID_CAP", &Options::grid_cap, nullptr},
  {"variant_rows", "GFFT_VARIANT_ROWS", &Options::variant_rows, nullptr},
  {"variant_cols", "GFFT_VARIANT_COLS", &Options::variant_cols, nullptr},
  {"force_generic", "GFFT_FORCE_GENERIC", &Options::force_generic, nullptr},
  {"copy_nt", nullptr, nullptr, &g_copy_nt},
  {"fused3", "GFFT_FUSED3", &Options::fused3, nullptr},
  {"plane2d", nullptr, &Options::plane2d, nullptr},
  {"fuse2", "GFFT_FUSE2", &Options::fuse2, nullptr},
  {"fuse2_ring", "GFFT_FUSE2_RING", &Options::fuse2_ring, nullptr},
  {"fuse2_lag", "GFFT_FUSE2_LAG", &Options::fuse2_lag, nullptr},
  {"fuse2_kinds", "GFFT_FUSE2_KINDS", &Options::fuse2_kinds, nullptr},
  {"fuse2_wait_ms", "GFFT_FUSE2_WAIT_MS", &Options::fuse2_wait_ms, nullptr},
  {"fuse2_f32", nullptr, &Options::fuse2_f32, nullptr},
  {"fuse2_n512", nullptr, nullptr, &g_fuse2_n512},
  {"c2r_2048", nullptr, nullptr, &g_c2r_2048},
  {"fuse2_mixv", nullptr, nullptr, &g_fuse2_mixv},
  {"fuse2_mixed", nullptr, nullptr, &g_fuse2_mixed},
  {"fuse2_f32_n512", nullptr, nullptr, &g_fuse2_f32_n512},
  {"debug_flat", nullptr, &Options::debug_flat, nullptr},
  {"flat_out", nullptr, &Options::flat_out, nullptr},
  {"wtile", nullptr, &Options::wtile, nullptr},
  {"mixv", nullptr, &Options::mixv, nullptr},
  {"mixv_variant", nullptr, &Options::mixv_variant, nullptr},
  {"debug_tile_lg", nullptr, &Options::debug_tile_lg, nullptr},
  {"debug_tile_side", nullptr, &Options::debug_tile_side, nullptr},
  {"debug_tile_stride", nullptr, &Options::debug_tile_stride, nullptr},
  {"profile", nullptr, &Options::profile, nullptr},
  {"debug_tw_index", nullptr, &Options::debug_tw_index, nullptr},
  {"debug_tw_exp", nullptr, &Options::debug_tw_exp, nullptr},
  {"debug_tw_len", nullptr, &Options::debug_tw_len, nullptr},
  {"debug_r2r_index", nullptr, &Options::debug_r2r_index, nullptr},
  {"debug_r2r_exp", nullptr, &Options::debug_r2r_exp, nullptr},
  {"debug_r2r_post", nullptr, &Options::debug_r2r_post, nullptr},
  {"xcd_swizzle", "GFFT_XCD_SWIZZLE", &Options::xcd_swizzle, nullptr},
  {"tile_order", nullptr, &Options::tile_order, nullptr},
};

// ---- one statement of each rule the creators and setters share ------------------------------------------------
// A plan in the making: the options a plan keeps from the moment it was made.  It dies with its owner on every error path ...
std::unique_ptr<gfft_plan_s> new_plan(int ndims, int kind, int precision) {
  std::unique_ptr<gfft_plan_s> pl(new gfft_plan_s);
  pl->ndims = ndims;  pl->kind = kind;  pl->precision = precision;
  pl->variant_rows = opts().variant_rows;  pl->variant_cols = opts().variant_cols;
  pl->mixv_variant = opts().mixv_variant;  pl->xcd_swizzle = opts().xcd_swizzle;
  return pl;
}
// ... or becomes the caller's handle: from here on gfft_plan_destroy is the one place it dies
int publish(gfft_plan *out, std::unique_ptr<gfft_plan_s> pl) {
  *out = pl.release();
  ++g_live_plans;
  return GFFT_OK;
}

int check_precision(int precision) {
  return precision == GFFT_F32 || precision == GFFT_F64 ? GFFT_OK : fail(GFFT_ERR_INVALID, "precision must be 4 or 8");
}

// one entry of an axes list: negative counts from the end; every axis at most once (seen: ndims flags)
int normalise_axis(int *a, int ndims, std::vector<char> *seen) {
  if (*a < 0) *a += ndims;
  if (*a < 0 || *a >= ndims || (*seen)[*a]) return fail(GFFT_ERR_INVALID, "bad or repeated axis");
  (*seen)[*a] = 1;
  return GFFT_OK;
}

// Blocks a transformed axis of length n may be cut into (the packed layouts of all-to-all buffers): a block is whole thread
// slots of the line's kernel -- R = 4 (n = 16), 8 or 16 (other powers of two), 12 / 20 (3^b 2^k / 5^c 2^k)
int max_split_blocks(int64_t n) { return is_pow2(n) ? (n >= 32 ? 8 : 4) : 4; }

// d_in == d_out: a workgroup loads its whole tile before it stores it, so a pass from the caller's input to the caller's
// output may run in place exactly when every tile writes the addresses it read.  That holds for the natural layouts and
// for the same re-laid-out form on both sides; it fails where gfft_plan_set_split / _set_tiles / _set_flat (body + leftover
// columns), guru blocks or a fused truncation / zero padding give the two sides different places for the same entry.
// (`in` is the pass that reads the caller's input, `out` the one that writes the caller's output: the same PassDesc, or the
// two halves of a fused pair.)
bool same_relayout(const PassDesc &in, const PassDesc &out) {
  return in.in_lgp == out.out_lgp && in.in_jump == out.out_jump && in.in_tlg == out.out_tlg && in.in_tS == out.out_tS &&
         in.in_ilg == out.out_ilg && in.in_iS == out.out_iS && !in.tr_dir && !out.tr_dir && !in.tr_jump && !out.tr_jump &&
         !in.ub_p && !out.ub_p && !in.fl_bw && !out.fl_bw;
}
bool in_place_ok(const gfft_plan_s *pl) {
  for (const Pass &p : pl->passes) {
    if (p.kind == PK_FUSED2 && p.src == BUF_IN && p.dst == BUF_OUT && !same_relayout(p.d, p.d2)) return false;
    if (p.kind == PK_FFT && p.src == BUF_IN && p.dst == BUF_OUT && (!same_relayout(p.d, p.d) || p.blocks[0] != p.blocks[1] || p.bstride[0] != p.bstride[1]))
      return false;
  }
  return true;
}

std::string misaligned(const char *name, size_t need, bool as_pair) {
  return std::string(name) + " must be aligned to " + std::to_string(need) + " bytes (" +
         (as_pair ? "a fused real pass pair addresses its real side as complex pairs" : "one element of the array") + ")";
}

}  // namespace

gfft::Options::Options() {
  for (const OptionRow &r : kOptions)
    if (const char *s = r.env ? getenv(r.env) : nullptr) this->*r.field = atoi(s);
}

extern "C" {

const char *gfft_strerror(int status) {
  switch (status) {
    case GFFT_OK: return "success";
    case GFFT_ERR_INVALID: return "invalid argument";
    case GFFT_ERR_UNSUPPORTED: return "unsupported transform";
    case GFFT_ERR_NO_DEVICE: return "no HIP device";
    case GFFT_ERR_HIP: return "HIP runtime error";
    case GFFT_ERR_NOMEM: return "out of memory";
    case GFFT_ERR_VOIDED: return "asynchronous launch failure";
  }
  return "unknown gfft status";
}

int gfft_version(void) { return 100; }

int gfft_device_count(int *count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    if (count) *count = 0;
    return fail(GFFT_ERR_NO_DEVICE, "no HIP device available");
  }
  if (count) *count = n;
  return GFFT_OK;
}

int gfft_device_name(int device, char *buf, size_t len) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return GFFT_OK;
}

int gfft_set_option(const char *key, int value) {
  if (!key) return fail(GFFT_ERR_INVALID, "null option name");
  if (!strcmp(key, "fused3_min_mib")) { opts().fused3_min_bytes = (int64_t)value << 20; return GFFT_OK; }
  for (const OptionRow &r : kOptions)
    if (!strcmp(key, r.key)) { (r.global ? *r.global : opts().*r.field) = value; return GFFT_OK; }
  return fail(GFFT_ERR_INVALID, std::string("unknown option ") + key);
}

int gfft_plan_create(gfft_plan *plan, int ndims, const int64_t *sizes_in, const int64_t *sizes_out,
                     int naxes, const int *axes, int kind, int precision) {
  if (!plan || !sizes_in || !sizes_out || !axes) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (ndims < 1 || ndims > 16 || naxes < 1 || naxes > ndims) return fail(GFFT_ERR_INVALID, "bad ndims/naxes");
  if (int bad = check_precision(precision)) return bad;
  if (kind != GFFT_C2C_FORWARD && kind != GFFT_C2C_BACKWARD && kind != GFFT_R2C && kind != GFFT_C2R)
    return fail(GFFT_ERR_UNSUPPORTED, "only c2c / r2c / c2r kinds are implemented (r2r kinds are out of scope)");
  std::vector<int> ax(axes, axes + naxes);
  std::vector<char> seen(ndims, 0);
  for (int &a : ax)
    if (int bad = normalise_axis(&a, ndims, &seen)) return bad;
  const int last = ax.back();
  for (int i = 0; i < ndims; ++i) {
    if (sizes_in[i] < 1 || sizes_out[i] < 1) return fail(GFFT_ERR_INVALID, "sizes must be >= 1");
    if (i == last && kind == GFFT_R2C) {
      if (sizes_out[i] != sizes_in[i] / 2 + 1) return fail(GFFT_ERR_INVALID, "r2c: sizes_out[axis] must be n/2+1");
    } else if (i == last && kind == GFFT_C2R) {
      if (sizes_in[i] != sizes_out[i] / 2 + 1) return fail(GFFT_ERR_INVALID, "c2r: sizes_in[axis] must be n/2+1");
    } else if (sizes_in[i] != sizes_out[i]) {
      return fail(GFFT_ERR_INVALID, "sizes_in and sizes_out may differ only along the halved axis");
    }
  }
  int rc = check_device();
  if (rc) return rc;

  auto owner = new_plan(ndims, kind, precision);
  gfft_plan_s *pl = owner.get();
  pl->sizes_in.assign(sizes_in, sizes_in + ndims);
  pl->sizes_out.assign(sizes_out, sizes_out + ndims);
  pl->axes = ax;

  rc = GFFT_OK;
  auto line = [&](int axis, int mode, bool inverse, const std::vector<int64_t> &sin_,
                  const std::vector<int64_t> &sout_, int src, int dst) {
    Line L;
    L.outer = L.inner = 1;
    for (int i = 0; i < axis; ++i) L.outer *= sin_[i];
    for (int i = axis + 1; i < ndims; ++i) L.inner *= sin_[i];
    L.nin = sin_[axis];
    L.nout = sout_[axis];
    L.n = (mode == MODE_C2R) ? sout_[axis] : sin_[axis];
    L.mode = mode;
    L.inverse = inverse;
    L.src = src;
    L.dst = dst;
    return plan_line(pl, L, true);
  };
  if (fused3_applicable(pl)) {
    rc = plan_fused3(pl);
  } else if (kind == GFFT_C2C_FORWARD || kind == GFFT_C2C_BACKWARD) {
    const bool inv = kind == GFFT_C2C_BACKWARD;
    for (int i = naxes - 1; i >= 0 && !rc; --i)
      rc = line(ax[i], MODE_C2C, inv, pl->sizes_in, pl->sizes_in, i == naxes - 1 ? BUF_IN : BUF_OUT, BUF_OUT);
    // Batched 2-D transforms over the last two axes of a 3-D array -- the leading stage of a slab-decomposed
    // PFFT with collapse=True, or fftn(axes=(1, 2)) --: plane by plane in one fused launch, [strided along axis 1 ->
    // rows along axis 2] in both directions (build_pair2d: strided reads, whole rows written -- round 6; against the
    // [rows -> strided] order of rounds 4-5: level in complex128, 9 % ahead in complex64, profiles/r06_stage_probe_slab.txt)
    if (!rc && ndims == 3 && naxes == 2 && ax[0] == 1 && ax[1] == 2 && pl->passes.size() == 2) {
      const Pass &pr = pl->passes[0], &pc = pl->passes[1];
      const int64_t n0 = sizes_in[0], n1 = sizes_in[1], n2 = sizes_in[2];
      if (pr.kind == PK_FFT && pc.kind == PK_FFT && pr.regk && pc.regk && !pr.cols && pc.cols && !pr.d.tw_hi && !pc.d.tw_hi &&
          is_pow2(n1) && is_pow2(n2) && n0 < ((int64_t)1 << 30)) {
        const std::vector<Pass> two = pl->passes;
        pl->passes.clear();
        const gfft_iodim c{n1, n2, n2}, p{n0, n1 * n2, n1 * n2};
        bool fused = false;
        if (build_pair2d(pl, &c, n2, &p, inv, 1, 1, 0, 1, 0, true, &fused) != GFFT_OK || !fused) pl->passes = two;
      }
    }
    // Planes of 32 x 32 / 64 x 64 points -- config C1's 64^3, small images --: rows and columns of a plane in ONE launch with the
    // plane held in LDS (fft_plane2d.hip): such arrays live in the caches and a pass costs its dependent memory round trip, not
    // its bytes (64^3 complex128: three passes of ~5 us each, tools/c1_probe.py); this removes one of them.
    // (a 2-D array is one plane)
    const int p0 = ndims - 2;                                // the two in-plane axes: p0, p0 + 1
    if (!rc && (ndims == 3 || ndims == 2) && naxes >= 2 && ax[naxes - 2] == p0 && ax[naxes - 1] == p0 + 1 &&
        (naxes == 2 || (ndims == 3 && naxes == 3 && ax[0] == 0)) &&
        sizes_in[p0] == sizes_in[p0 + 1] && plane2d_supported((int)sizes_in[p0], precision) && pl->passes.size() == (size_t)naxes && opts().plane2d) {
      const Pass &pr = pl->passes[0], &pc = pl->passes[1];
      const int64_t nplanes = ndims == 3 ? sizes_in[0] : 1;
      if (pr.kind == PK_FFT && pc.kind == PK_FFT && pr.regk && pc.regk && !pr.cols && pc.cols && nplanes < ((int64_t)1 << 30)) {
        const int64_t n = sizes_in[p0], P = plane2d_pitch((int)n), esz = 2 * (int64_t)precision;
        Pass f = pr;
        f.kind = PK_PLANE2D;
        f.d = pr.d;                                          // rows of ONE plane: natural rows -> the plane in LDS, rows P entries apart
        f.d.batch = n;  f.d.mid = 1;  f.d.inner = 1;  f.d.in_os = n;  f.d.in_is = 0;  f.d.out_os = P;  f.d.out_is = 0;
        f.d2 = pc.d;                                         // columns of one plane: LDS -> natural rows
        f.d2.batch = n;  f.d2.mid = 1;  f.d2.inner = n;  f.d2.in_os = 0;  f.d2.out_os = 0;  f.d2.in_es = P;  f.d2.in_is = 1;
        f.fused.planes = (int)nplanes;
        f.fused.a_in_plane = n * n * esz;
        f.fused.b_out_plane = n * n * esz;
        f.src = BUF_IN;  f.dst = BUF_OUT;
        f.bytes2 = 4.0 * (double)nplanes * (double)n * (double)n * (double)esz;
        pl->passes.erase(pl->passes.begin(), pl->passes.begin() + 2);
        pl->passes.insert(pl->passes.begin(), f);
      }
    }
  } else if (kind == GFFT_R2C) {
    rc = line(last, MODE_R2C, false, pl->sizes_in, pl->sizes_out, BUF_IN, BUF_OUT);
    for (int i = naxes - 2; i >= 0 && !rc; --i)
      rc = line(ax[i], MODE_C2C, false, pl->sizes_out, pl->sizes_out, BUF_OUT, BUF_OUT);
  } else {
    // C2R: the complex passes run into / inside the WS region, so the caller's input is never
    // written (FFTW's multi-dimensional c2r destroys it), then the real pass
    for (int i = 0; i <= naxes - 2 && !rc; ++i)
      rc = line(ax[i], MODE_C2C, true, pl->sizes_in, pl->sizes_in, i == 0 ? BUF_IN : BUF_WS, BUF_WS);
    if (!rc) rc = line(last, MODE_C2R, true, pl->sizes_in, pl->sizes_out, naxes > 1 ? BUF_WS : BUF_IN, BUF_OUT);
    if (naxes > 1) {
      size_t bytes = 2 * (size_t)precision;
      for (int i = 0; i < ndims; ++i) bytes *= (size_t)sizes_in[i];
      need(pl, BUF_WS, bytes);
    }
  }
  if (rc) return rc;
  // the scale factor rides on the last pass
  pl->passes.back().carries_scale = true;
  return publish(plan, std::move(owner));
}

int gfft_plan_create_padded(gfft_plan *plan, const int64_t *padded, const int64_t *kept, int kind, int precision) {
  if (!plan || !padded || !kept) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (int bad = check_precision(precision)) return bad;
  if (kind != GFFT_C2C_FORWARD && kind != GFFT_C2C_BACKWARD && kind != GFFT_R2C && kind != GFFT_C2R)
    return fail(GFFT_ERR_INVALID, "kind must be c2c forward / backward, r2c or c2r");
  const bool real = kind == GFFT_R2C || kind == GFFT_C2R;
  const bool inverse = kind == GFFT_C2C_BACKWARD || kind == GFFT_C2R;
  for (int i = 0; i < 3; ++i) {
    const int64_t of = (real && i == 2) ? padded[i] / 2 + 1 : padded[i];
    if (padded[i] < 1 || kept[i] < 1 || kept[i] > of) return fail(GFFT_ERR_INVALID, "kept entries must lie in 1 .. transformed entries");
  }
  int rc = check_device();
  if (rc) return rc;
  // the all-axes schedule needs one register-kernel pass per axis (packed-real rows on a real axis)
  if (!opts().fused3) return fail(GFFT_ERR_UNSUPPORTED, "fused 3-D plans are switched off");
  for (int i = 0; i < 3; ++i) {
    const bool real_axis = i == 2 && real;
    const bool one_pass = regk_ok(padded[i], precision) ||
                          (real_axis ? (padded[i] % 2 == 0 && real_half_mixv_ok(padded[i] / 2)) : regk_c2c_ok(padded[i], precision, MODE_C2C));
    if (!one_pass || (kept[i] < (real_axis ? padded[i] / 2 + 1 : padded[i]) && !fused_pad_ok(real_axis ? padded[i] / 2 : padded[i])))
      return fail(GFFT_ERR_UNSUPPORTED, "padded length without a single-pass kernel");
  }
  if (real && !(padded[2] % 2 == 0 &&
                (real_half_supported((int)(padded[2] / 2)) || real_half_mix_supported((int)(padded[2] / 2)) || real_half_mixv_ok(padded[2] / 2))))
    return fail(GFFT_ERR_UNSUPPORTED, "real axis without a packed-real row kernel");
  const int64_t bytes = padded[0] * padded[1] * padded[2] * (real ? 1 : 2) * precision;
  if (bytes < opts().fused3_min_bytes) return fail(GFFT_ERR_UNSUPPORTED, "below the size where the workspace schedule pays");
  auto pl = new_plan(3, kind, precision);
  std::vector<int64_t> phys(padded, padded + 3), spec(kept, kept + 3);
  pl->sizes_in = inverse ? spec : phys;
  pl->sizes_out = inverse ? phys : spec;
  pl->axes = {0, 1, 2};
  pl->trunc = spec;
  rc = plan_fused3(pl.get());
  if (rc) return rc;
  pl->passes.back().carries_scale = true;
  return publish(plan, std::move(pl));
}

int gfft_plan_create_r2r(gfft_plan *plan, int ndims, const int64_t *sizes, int naxes, const int *axes,
                         const int *kinds, int precision) {
  if (!plan || !sizes || !axes || !kinds) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (ndims < 1 || ndims > 16 || naxes < 1 || naxes > ndims) return fail(GFFT_ERR_INVALID, "bad ndims/naxes");
  if (int bad = check_precision(precision)) return bad;
  std::vector<int> ax(axes, axes + naxes);
  std::vector<char> seen(ndims, 0);
  for (int i = 0; i < naxes; ++i) {
    if (int bad = normalise_axis(&ax[i], ndims, &seen)) return bad;
    if (kinds[i] < GFFT_REDFT00 || kinds[i] > GFFT_RODFT11)
      return fail(GFFT_ERR_UNSUPPORTED, "r2r kind must be one of REDFT00..RODFT11 (halfcomplex / DHT kinds are not implemented)");
  }
  for (int i = 0; i < ndims; ++i)
    if (sizes[i] < 1) return fail(GFFT_ERR_INVALID, "sizes must be >= 1");
  int rc = check_device();
  if (rc) return rc;
  auto pl = new_plan(ndims, GFFT_R2R, precision);
  pl->sizes_in.assign(sizes, sizes + ndims);
  pl->sizes_out = pl->sizes_in;
  pl->axes = ax;
  for (int i = naxes - 1; i >= 0 && !rc; --i) {
    int64_t outer = 1, inner = 1;
    for (int k = 0; k < ax[i]; ++k) outer *= sizes[k];
    for (int k = ax[i] + 1; k < ndims; ++k) inner *= sizes[k];
    rc = plan_r2r_line(pl.get(), outer, sizes[ax[i]], inner, kinds[i], i == naxes - 1 ? BUF_IN : BUF_OUT, BUF_OUT);
  }
  if (rc) return rc;
  pl->passes.back().carries_scale = true;
  return publish(plan, std::move(pl));
}

int gfft_execute(gfft_plan pl, const void *d_in, void *d_out, double scale, void *stream) {
  if (!pl || !d_in || !d_out) return fail(GFFT_ERR_INVALID, "null argument");
  {
    // a fused launch of an earlier execution of THIS plan gave up a wait: report it now, once, and enqueue nothing (the
    // plan has been switched to stand-alone passes; calling again runs it that way).  Another plan's pending event stays
    // with that plan (gfft_plan_status / gfft_async_error / its own next execute) and does not refuse this call.
    int rc = poll_async_error(pl);
    if (rc) return rc;
  }
  if (current_device() != pl->device) return fail(GFFT_ERR_INVALID, "the plan was made on another device than the calling thread's current one");
  if ((pl->kind == GFFT_R2C || pl->kind == GFFT_C2R) && d_in == d_out)
    return fail(GFFT_ERR_INVALID, "in-place real transforms are not supported");
  if (d_in == d_out && !in_place_ok(pl))
    return fail(GFFT_ERR_INVALID, "in-place execution needs the same layout on both sides (this plan re-lays one side out: a tile would overwrite input that another tile has yet to read)");
  {
    // Base alignment (include/gfft.h).  The kernels address their arrays element by element -- cx<real> is two reals and is
    // aligned as ONE --, so an array need only be aligned as an element of its own type.  The exceptions are the non-temporal
    // streams (fft_pow2_impl.h ldc / stc), typed as a vector of two reals: on a complex array that is the element again; the
    // real side of a fused real pair, which they read / write as complex pairs, must be aligned as a pair.
    const size_t prec = (size_t)pl->precision;
    const bool in_real = pl->kind == GFFT_R2C || pl->kind == GFFT_R2R, out_real = pl->kind == GFFT_C2R || pl->kind == GFFT_R2R;
    bool pair = false;
    for (const Pass &q : pl->passes) pair = pair || q.kind == PK_FUSED2;
    const bool pair_in = pair && pl->kind == GFFT_R2C, pair_out = pair && pl->kind == GFFT_C2R;
    const size_t a_in = (in_real && !pair_in) ? prec : 2 * prec, a_out = (out_real && !pair_out) ? prec : 2 * prec;
    if ((uintptr_t)d_in % a_in) return fail(GFFT_ERR_INVALID, misaligned("d_in", a_in, pair_in));
    if ((uintptr_t)d_out % a_out) return fail(GFFT_ERR_INVALID, misaligned("d_out", a_out, pair_out));
  }
  if (!pl->fused_off && pl->async_slot < 0) {
    bool any = false;
    for (const Pass &q : pl->passes) any = any || q.kind == PK_FUSED2;
    if (any) {
      // this plan's own word of the host-visible table: two live plans never share one (ids 64 apart used to), so a
      // voided launch is always attributed; with every word taken the pairs run as their stand-alone passes instead
      AsyncErrors &ae = async_errors();
      std::lock_guard<std::mutex> lock(ae.m);
      if (ae.word())
        for (int i = 0; i < AsyncErrors::SLOTS && pl->async_slot < 0; ++i)
          if (!ae.owner[i]) { ae.owner[i] = pl; pl->async_slot = i; }
      if (pl->async_slot < 0) fused_pairs_off(pl);
    }
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // scratch regions: carved from the stream's shared buffer (scratch_pool)
  size_t off[BUF_COUNT] = {0, 0, 0, 0, 0, 0, 0}, total = 0;
  for (int b = BUF_WS; b < BUF_COUNT; ++b) {
    off[b] = total;
    total += align256(pl->region_bytes[b]);
  }
  void *scratch = nullptr;
  if (total) {
    int rc = scratch_pool().get(s, total, &scratch);
    if (rc) return rc;
  }
  void *bufs[BUF_COUNT] = {const_cast<void *>(d_in), d_out, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int b = BUF_WS; b < BUF_COUNT; ++b)
    if (pl->region_bytes[b]) bufs[b] = static_cast<char *>(scratch) + off[b];

  std::vector<hipEvent_t> *ev = nullptr;
  auto mark = [&]() -> hipError_t {
    if (!ev) return hipSuccess;
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return rc;
    rc = hipEventRecord(e, s);
    ev->push_back(e);
    return rc;
  };
  if (opts().profile) {
    pl->prof.emplace_back();
    ev = &pl->prof.back();
    HIP_TRY(mark());
  }
  for (const Pass &p : pl->passes) {
    PassDesc d = p.d;
    if (p.kind == PK_PLANE2D) {
      PassDesc d2 = p.d2;
      d2.scale = p.carries_scale ? scale : 1.0;
      last_launch() = LaunchNote{};
      HIP_TRY(launch_plane2d(d, d2, pl->precision, p.fused.planes, p.fused.a_in_plane, p.fused.b_out_plane, bufs[p.src], bufs[p.dst], s));
      p.launched = last_launch();
      HIP_TRY(mark());
      continue;
    }
    if (p.kind == PK_FUSED2 && pl->fused_off) {
      // the pair as its two stand-alone passes (a fused launch of this plan gave up a wait, poll_async_error)
      for (int k = 0; k < 2; ++k) {
        const Pass &q = pl->alt[p.alt_first + k];
        PassDesc dq = q.d;
        const bool sc = k == 1 && p.carries_scale;
        if (sc) dq.scale = scale;
        HIP_TRY(run_pass(pl, q, dq, bufs[q.src], bufs[q.dst], sc ? scale : 1.0, s));
      }
      HIP_TRY(mark());
      continue;
    }
    if (p.kind == PK_FUSED2) {
      PassDesc d2 = p.d2;
      if (p.carries_scale) d2.scale = scale;
      FusedDesc f = p.fused;
      char *ring = static_cast<char *>(bufs[BUF_RING]);
      f.ctr = reinterpret_cast<unsigned *>(ring + (size_t)f.ring * (size_t)f.slot_bytes);
      {
        AsyncErrors &ae = async_errors();
        f.host_flag = (ae.flag && pl->async_slot >= 0) ? ae.flag + pl->async_slot : nullptr;
        const int ms = opts().fuse2_wait_ms;
        f.wait_ticks = ms <= 0 ? 0u : (ms > 40000 ? 4000000000u : (unsigned)ms * 100000u);      // 100 MHz ticks
      }
      static const int debug = getenv("GFFT_FUSE2_DEBUG") ? atoi(getenv("GFFT_FUSE2_DEBUG")) : 0;
      if (debug) { f.wait_ticks = 100000u; f.host_flag = nullptr; f.debug = (unsigned)debug; }      // (1 ms; counters printed below)
      HIP_TRY(p.pair->launch(d, d2, p.dev_descs, f, bufs[p.src], ring, bufs[p.dst], s));
      if (debug) {      // developer aid: the launch's counters (tickets drawn, waits given up, tiles per plane)
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<unsigned> h(16 + 2 * (size_t)f.planes);
        HIP_TRY(hipMemcpy(h.data(), f.ctr, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        unsigned long long sa = 0, sb = 0;
        for (int i = 0; i < f.planes; ++i) { sa += h[16 + i]; sb += h[16 + f.planes + i]; }
        fprintf(stderr, "[gfft fuse2] kind %d planes %d tiles %d+%d ring %d lag %d: tickets %u, waits given up %u, A tiles %llu, B tiles %llu\n",
                p.fused_kind, f.planes, f.tiles_a, f.tiles_b, f.ring, f.lag, h[0], h[1], sa, sb);
#ifdef GFFT_FUSE2_TRACE
        if (const char *path = getenv("GFFT_FUSE2_TRACE_FILE")) {
          std::vector<unsigned long long> tr((size_t)1024 * 96 * 16);
          const size_t off = ((16 + 2 * (size_t)f.planes + 63) & ~(size_t)63) * sizeof(unsigned);
          HIP_TRY(hipMemcpy(tr.data(), reinterpret_cast<char *>(f.ctr) + off, tr.size() * sizeof(tr[0]), hipMemcpyDeviceToHost));
          if (FILE *fp = fopen(path, "wb")) { fwrite(tr.data(), sizeof(tr[0]), tr.size(), fp); fclose(fp); }
        }
#endif
      }
      HIP_TRY(mark());
      continue;
    }
    if (p.carries_scale) d.scale = scale;
    last_launch() = LaunchNote{};
    HIP_TRY(run_pass(pl, p, d, bufs[p.src], bufs[p.dst], p.carries_scale ? scale : 1.0, s));
    p.launched = last_launch();      // (gfft_plan_pass_launch)
    HIP_TRY(mark());
  }
  return GFFT_OK;
}

/* Accumulated per-pass kernel time since the last call (needs option "profile" = 1 while
 * executing): ms[i] = total milliseconds of pass i, *executes = number of executes summed.
 * Synchronises on the recorded events and frees them. */
int gfft_plan_profile(gfft_plan pl, float *ms, int max_passes, int *executes) {
  if (!pl || !ms) return fail(GFFT_ERR_INVALID, "null argument");
  for (int i = 0; i < max_passes; ++i) ms[i] = 0.f;
  int n = 0;
  for (auto &ev : pl->prof) {
    if (ev.empty()) continue;
    HIP_TRY(hipEventSynchronize(ev.back()));
    for (size_t i = 0; i + 1 < ev.size(); ++i) {
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      if ((int)i < max_passes) ms[i] += t;
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ++n;
  }
  pl->prof.clear();
  if (executes) *executes = n;
  return GFFT_OK;
}

/* text name of the kernel family behind pass i ("pow2-rows", "pow2-cols", "generic") */
int gfft_plan_pass_info(gfft_plan pl, int i, char *buf, size_t len, double *bytes) {
  if (!pl || i < 0 || i >= (int)pl->passes.size()) return fail(GFFT_ERR_INVALID, "bad pass index");
  const Pass &p = pl->passes[i];
  static const char *kinds[] = {"", "embed", "mul-B", "extract"};
  if (p.kind == PK_FUSED2) {
    // two axis passes in one launch: the algorithmic bytes of both (one read + one write of the array each)
    snprintf(buf, len, "%s n=%dx%d", kFusedKinds[p.fused_kind].pass_name, p.d.n, p.d2.n);
    if (bytes) *bytes = p.bytes2 > 1 ? p.bytes2 : (double)p.fused.planes * 2.0 * pl->precision *
                        ((double)p.d.batch * 2.0 * p.d.n + (double)p.d2.batch * 2.0 * p.d2.n);
    return GFFT_OK;
  }
  if (p.kind == PK_PLANE2D) {
    snprintf(buf, len, "planes in LDS rows+cols n=%dx%d", p.d.n, p.d2.n);
    if (bytes) *bytes = p.bytes2;
    return GFFT_OK;
  }
  if (p.kind != PK_FFT) {
    snprintf(buf, len, "%s n=%lld", kinds[p.kind], (long long)p.pt.n);
    if (bytes) *bytes = 0;
    return GFFT_OK;
  }
  const bool percol = !p.regk && (p.d.n == 3 || p.d.n == 5 || p.d.n == 7 || p.d.n == 11 || p.d.n == 13) &&
                      p.d.mode == MODE_C2C && !p.d.tw_hi && p.d.in_is == 1 && p.d.out_is == 1 && p.d.inner >= 64;
  snprintf(buf, len, "%s n=%d", p.regk ? (p.cols ? "pow2-cols" : "pow2-rows") : (percol ? "percol" : "generic"), p.d.n);
  if (bytes && (p.d.mode == MODE_R2C_H || p.d.mode == MODE_C2R_H)) {
    // n complex = 2n reals on one side, n + 1 complex on the other
    *bytes = (double)p.d.batch * (2.0 * p.d.n * pl->precision + (p.d.n + 1.0) * 2.0 * pl->precision);
    snprintf(buf, len, "real-rows n=%d", 2 * p.d.n);
    return GFFT_OK;
  }
  if (bytes) {
    const double esz = 2.0 * pl->precision;
    const double nc = p.d.mode == MODE_C2C ? p.d.n : p.d.n / 2 + 1;
    const double ein = p.d.mode == MODE_R2C ? p.d.n * (double)pl->precision : nc * esz;
    const double eout = p.d.mode == MODE_C2R ? p.d.n * (double)pl->precision : nc * esz;
    *bytes = (double)p.d.batch * (ein + eout);
    if (p.data_inner) *bytes *= (double)p.data_inner / (double)p.d.inner;
    if (p.d.mode == MODE_R2R) *bytes = (double)p.d.batch * 2.0 * p.d.r2r_n * (double)pl->precision;
  }
  return GFFT_OK;
}

/* TEST AID: the launch form of pass i's most recent launch, as its launcher noted it (gfft_internal.h note_launch) */
int gfft_plan_pass_launch(gfft_plan pl, int i, int64_t *tiles, int *workgroups) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (!tiles || !workgroups) return fail(GFFT_ERR_INVALID, "null argument");
  if (i < 0 || i >= (int)pl->passes.size()) return fail(GFFT_ERR_INVALID, "bad pass index");
  const Pass &p = pl->passes[i];
  if (p.kind == PK_FUSED2) return fail(GFFT_ERR_UNSUPPORTED, "a persistent fused pair has no launch form to report (its workgroups draw tickets)");
  *tiles = p.launched.tiles;
  *workgroups = p.launched.workgroups;
  return GFFT_OK;
}

/* Fuse the 3/2-rule truncation (forward kinds) or zero-padding (backward kinds) of
 * libfft.py:263-311 into a single-axis plan: the truncated array (n_keep entries along the axis:
 * N for a complex axis, N/2+1 for the real half-axis) becomes the plan's output (input).
 * Returns GFFT_ERR_UNSUPPORTED, leaving the plan unchanged, when the plan is not one
 * register-kernel pass (the caller then uses gfft_truncate / gfft_pad). */
int gfft_plan_set_truncation(gfft_plan pl, int64_t n_keep) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (pl->passes.size() != 1 || pl->axes.size() != 1 || pl->fused3)
    return fail(GFFT_ERR_UNSUPPORTED, "truncation fuses into single-pass plans only");
  Pass &p = pl->passes[0];
  if (p.d.mode == MODE_R2C_H || p.d.mode == MODE_C2R_H) {
    // packed-real rows: the truncating store / zero-padding load act on the half spectrum
    // (entries 0 .. n_keep-1 of the p.d.n + 1; strides are in complex entries, inner == 1)
    const int64_t full_h = (int64_t)p.d.n + 1;
    if (n_keep < 1 || n_keep > full_h) return fail(GFFT_ERR_INVALID, "bad truncated length");
    if (n_keep == full_h) return GFFT_OK;        // nothing to cut: the plain plan is the answer
    if (!fused_pad_ok(p.d.n)) return fail(GFFT_ERR_UNSUPPORTED, "no fused truncation kernels for this length in this build");
    const bool fwd_h = p.d.mode == MODE_R2C_H;
    const double lines_h = (double)p.d.batch, esz_h = 2.0 * pl->precision;
    (fwd_h ? p.d.out_os : p.d.in_os) = n_keep;
    pl->bytes += lines_h * ((double)n_keep - (double)full_h) * esz_h;
    set_truncation(p.d, fwd_h ? 1 : 2, n_keep);
    return GFFT_OK;
  }
  if (p.kind != PK_FFT || !p.regk || p.d.mid != 1 || p.d.tw_hi || !fused_pad_ok(p.d.n))
    return fail(GFFT_ERR_UNSUPPORTED, "truncation fuses into register-kernel passes only");
  const int axis = pl->axes[0];
  const bool fwd = pl->kind == GFFT_C2C_FORWARD || pl->kind == GFFT_R2C;
  const bool real = pl->kind == GFFT_R2C || pl->kind == GFFT_C2R;
  const int64_t full = real ? p.d.n / 2 + 1 : p.d.n;
  if (n_keep < 1 || n_keep > full) return fail(GFFT_ERR_INVALID, "bad truncated length");
  int64_t inner = 1;
  for (int i = axis + 1; i < pl->ndims; ++i) inner *= pl->sizes_in[i];
  const double esz = 2.0 * pl->precision;
  const double lines = (double)p.d.batch;
  (fwd ? p.d.out_os : p.d.in_os) = n_keep * inner;
  pl->bytes -= lines * (double)full * esz;
  pl->bytes += lines * (double)n_keep * esz;
  set_truncation(p.d, fwd ? 1 : 2, n_keep);
  return GFFT_OK;
}

/* Packed-layout adapters (see include/gfft.h).  side 0: the plan reads its input from an
 * all-to-all receive buffer; side 1: it writes its output as an all-to-all send buffer.  Both are
 * the layout gfft_pack produces for `nblocks` equal blocks of the transformed axis:
 * [block][outer][n/nblocks][inner].  nblocks = 1 restores the natural layout. */
int gfft_plan_set_split(gfft_plan pl, int side, int nblocks) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (side != 0 && side != 1) return fail(GFFT_ERR_INVALID, "side must be 0 (input) or 1 (output)");
  if (pl->passes.size() != 1 || pl->axes.size() != 1 || pl->fused3)
    return fail(GFFT_ERR_UNSUPPORTED, "split layouts fuse into single-pass plans only");
  Pass &p = pl->passes[0];
  // (3 x 5 x 2^k lengths: their stages keep different numbers of values per thread, and a block boundary would have to
  // fall between the same thread slots on the load AND the store geometry -- natural layouts only, fft_mixv_*.hip)
  if (p.regk && mixv_supported(p.d.n)) return fail(GFFT_ERR_UNSUPPORTED, "split layouts: not for 3 x 5 x 2^k lengths");
  if ((p.d.mode == MODE_R2C_H && side == 1) || (p.d.mode == MODE_C2R_H && side == 0)) {
    // packed-real rows: the half-spectrum side as an all-to-all buffer of UNEVEN blocks (the
    // n/2 + 1 entries never divide evenly; pencil.py:5-9 deals the remainder to the first ranks)
    if (p.d.mid != 1 || p.d.inner != 1) return fail(GFFT_ERR_UNSUPPORTED, "split layout: packed-real rows only");
    // (with a fused truncation / zero padding the blocks are those of the KEPT entries)
    const int nh = p.d.tr_dir ? p.d.tr_n : p.d.n + 1;
    if (nblocks < 1 || nblocks > 8 || nblocks > nh) return fail(GFFT_ERR_UNSUPPORTED, "split layout: at most 8 blocks");
    if (nblocks == 1) {
      p.d.ub_p = 0;
      return GFFT_OK;
    }
    const int q = nh / nblocks, r = nh % nblocks;
    p.d.ub_p = nblocks;
    for (int b = 0; b <= nblocks; ++b) p.d.ub_start[b] = b * q + (b < r ? b : r);
    for (int b = nblocks + 1; b < 9; ++b) p.d.ub_start[b] = nh;
    p.d.ub_minw = q;
    p.d.ub_rows = p.d.batch;
    return GFFT_OK;
  }
  if (p.kind != PK_FFT || !p.regk || p.d.mid != 1 || p.d.tw_hi || p.d.mode != MODE_C2C)
    return fail(GFFT_ERR_UNSUPPORTED, "split layouts fuse into complex register-kernel passes only");
  const int64_t n = p.d.n, inner = p.d.inner, outer = p.d.batch / p.d.inner;
  if (!is_pow2(nblocks)) return fail(GFFT_ERR_UNSUPPORTED, "block count must be a power of two");
  const int lg = ilog2_ceil(nblocks);
  if (p.d.tr_dir && side == (p.d.tr_dir == 1 ? 1 : 0)) {
    // the TRUNCATED side of a fused 3/2-rule truncation / zero padding: equal blocks of the kept
    // entries, addressed per entry (PassDesc::tr_jump) -- no tie to the kernel's thread layout
    const int64_t keep = p.d.tr_N;
    if (nblocks > 8 || keep % nblocks) return fail(GFFT_ERR_UNSUPPORTED, "block count does not divide the kept length");
    const int64_t per = keep / nblocks;
    if (nblocks > 1 && !is_pow2(per)) return fail(GFFT_ERR_UNSUPPORTED, "kept entries per block must be a power of two");
    if (nblocks > 1 && (double)(outer - 1) * per * inner * (nblocks - 1) >= 2147483648.0)
      return fail(GFFT_ERR_UNSUPPORTED, "blocked truncated side beyond 2^31 elements");      // (32-bit block offsets in the kernels)
    p.d.tr_lgper = nblocks > 1 ? ilog2_ceil(per) : 0;
    p.d.tr_jump = nblocks > 1 ? (outer - 1) * per * inner : 0;
    (side == 0 ? p.d.in_os : p.d.out_os) = per * inner;
    return GFFT_OK;
  }
  if (nblocks > max_split_blocks(n) || n % nblocks) return fail(GFFT_ERR_UNSUPPORTED, "block count not supported for this length");
  const int64_t nb = n / nblocks;
  const int64_t os = nb * inner, jump = nblocks > 1 ? (outer - 1) * nb * inner : 0;
  // (what gfft_plan_create_guru would have recorded for the same layout: gfft_plan_set_tiles re-derives the block
  // jump from these)
  p.blocks[side] = nblocks;
  p.bstride[side] = nblocks > 1 ? outer * nb * inner : 0;
  if (side == 0) {
    p.d.in_os = os;
    p.d.in_jump = jump;
    p.d.in_lgp = lg;
  } else {
    p.d.out_os = os;
    p.d.out_jump = jump;
    p.d.out_lgp = lg;
  }
  return GFFT_OK;
}

int gfft_plan_create_guru(gfft_plan *plan, int precision, int kind, const gfft_iodim *dim, int howmany_rank,
                          const gfft_iodim *howmany, int in_blocks, int64_t in_block_stride, int out_blocks,
                          int64_t out_block_stride) {
  return gfft_plan_create_guru_padded(plan, precision, kind, dim, 0, howmany_rank, howmany, in_blocks, in_block_stride,
                                      out_blocks, out_block_stride);
}

int gfft_plan_create_guru_padded(gfft_plan *plan, int precision, int kind, const gfft_iodim *dim, int64_t n_keep,
                                 int howmany_rank, const gfft_iodim *howmany, int in_blocks, int64_t in_block_stride,
                                 int out_blocks, int64_t out_block_stride) {
  if (!plan || !dim || (howmany_rank > 0 && !howmany)) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (int bad = check_precision(precision)) return bad;
  if (kind != GFFT_C2C_FORWARD && kind != GFFT_C2C_BACKWARD) return fail(GFFT_ERR_UNSUPPORTED, "guru plans are complex-to-complex");
  if (howmany_rank < 0 || howmany_rank > 3) return fail(GFFT_ERR_UNSUPPORTED, "at most three batch dims");
  if (dim->n < 1) return fail(GFFT_ERR_INVALID, "bad transform length");
  int rc = check_device();
  if (rc) return rc;
  if (!regk_ok(dim->n, precision)) return fail(GFFT_ERR_UNSUPPORTED, "no single-pass register kernel for this length");
  // batch dims -> (outer, mid, inner): the last listed dim is the one adjacent columns run along
  gfft_iodim o{1, 0, 0}, m{1, 0, 0}, i{1, 0, 0};
  if (howmany_rank == 1) i = howmany[0];
  if (howmany_rank == 2) { o = howmany[0]; i = howmany[1]; }
  if (howmany_rank == 3) { o = howmany[0]; m = howmany[1]; i = howmany[2]; }
  if (o.n < 1 || m.n < 1 || i.n < 1) return fail(GFFT_ERR_INVALID, "bad batch length");
  const double batch = (double)o.n * (double)m.n * (double)i.n;
  if (batch >= 2147483648.0) return fail(GFFT_ERR_UNSUPPORTED, "batch exceeds 2^31");
  const int64_t n = dim->n;
  if (n_keep < 0 || n_keep > n) return fail(GFFT_ERR_INVALID, "bad kept length");
  const bool trunc = n_keep > 0 && n_keep < n;
  if (trunc && !fused_pad_ok(n)) return fail(GFFT_ERR_UNSUPPORTED, "no fused truncation kernels for this length in this build");
  const int tr_side = kind == GFFT_C2C_FORWARD ? 1 : 0;           // the side that holds the kept entries
  auto blocks_ok = [&](int nb, int side) {
    if (nb < 1 || (nb & (nb - 1))) return false;
    if (trunc && side == tr_side)                                // equal power-of-two blocks of the kept entries
      return nb <= 8 && n_keep % nb == 0 && (nb == 1 || is_pow2(n_keep / nb));
    return nb <= max_split_blocks(n) && n % nb == 0;
  };
  if (!blocks_ok(in_blocks, 0) || !blocks_ok(out_blocks, 1)) return fail(GFFT_ERR_UNSUPPORTED, "block count not supported for this length");
  auto pl = new_plan(0, kind, precision);
  Pass p;
  p.regk = true;
  p.cols = !(dim->is == 1 && dim->os == 1);
  p.logical_first = true;
  p.carries_scale = true;
  PassDesc &d = p.d;
  const bool inverse = kind == GFFT_C2C_BACKWARD;
  d.n = (int)n;
  d.mode = MODE_C2C;
  d.conj_in = d.conj_out = inverse ? 1 : 0;
  d.batch = o.n * m.n * i.n;
  d.mid = m.n;
  d.inner = i.n;
  d.in_os = o.is; d.in_ms = m.is; d.in_is = i.is; d.in_es = dim->is;
  d.out_os = o.os; d.out_ms = m.os; d.out_is = i.os; d.out_es = dim->os;
  d.scale = 1.0;
  if (in_blocks > 1 && !(trunc && tr_side == 0)) { d.in_lgp = ilog2_ceil(in_blocks); d.in_jump = in_block_stride - (n / in_blocks) * dim->is; }
  if (out_blocks > 1 && !(trunc && tr_side == 1)) { d.out_lgp = ilog2_ceil(out_blocks); d.out_jump = out_block_stride - (n / out_blocks) * dim->os; }
  if (trunc) {
    // fused 3/2-rule truncation (forward: store side) / zero padding (backward: load side), as
    // gfft_plan_set_truncation sets it on natural plans; blocks of the kept entries by PassDesc::tr_jump
    set_truncation(d, tr_side == 1 ? 1 : 2, n_keep);
    const int nb = tr_side == 1 ? out_blocks : in_blocks;
    if (nb > 1) {
      const int64_t per = n_keep / nb;
      d.tr_lgper = ilog2_ceil(per);
      d.tr_jump = (tr_side == 1 ? out_block_stride - per * dim->os : in_block_stride - per * dim->is);
      if (std::fabs((double)d.tr_jump) * (nb - 1) >= 2147483648.0)        // (32-bit block offsets in the kernels)
        return fail(GFFT_ERR_UNSUPPORTED, "blocked truncated side beyond 2^31 elements");
    }
  }
  p.blocks[0] = in_blocks;   p.bstride[0] = in_block_stride;
  p.blocks[1] = out_blocks;  p.bstride[1] = out_block_stride;
  rc = get_twiddles(n, precision, &d.tw);
  if (rc) return rc;
  pl->passes.push_back(p);
  if (n > 1) pl->flops = 5.0 * (double)n * std::log2((double)n) * batch;
  pl->bytes = batch * (double)(n + (trunc ? n_keep : n)) * 2.0 * precision;
  return publish(plan, std::move(pl));
}

/* The two local stages of a slab-decomposed transform as one plan (see include/gfft.h). */
int gfft_plan_create_guru2(gfft_plan *plan, int precision, int kind, const gfft_iodim *cols, const gfft_iodim *rows,
                           const gfft_iodim *planes, int cols_first, int in_blocks, int64_t in_block_stride,
                           int out_blocks, int64_t out_block_stride) {
  if (!plan || !cols || !rows || !planes) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (int bad = check_precision(precision)) return bad;
  if (kind != GFFT_C2C_FORWARD && kind != GFFT_C2C_BACKWARD) return fail(GFFT_ERR_UNSUPPORTED, "guru plans are complex-to-complex");
  const int64_t n1 = cols->n, n2 = rows->n, np = planes->n;
  if (n1 < 1 || n2 < 1 || np < 1) return fail(GFFT_ERR_INVALID, "bad length");
  if (rows->is != 1 || rows->os != 1) return fail(GFFT_ERR_UNSUPPORTED, "the row axis must be contiguous on both sides");
  if (in_blocks < 1 || out_blocks < 1) return fail(GFFT_ERR_INVALID, "bad block count");
  if (in_blocks > 1 && out_blocks > 1) return fail(GFFT_ERR_UNSUPPORTED, "blocks on one side only");
  int rc = check_device();
  if (rc) return rc;
  if (!regk_ok(n1, precision) || !regk_ok(n2, precision) || mixv_supported((int)n1))
    return fail(GFFT_ERR_UNSUPPORTED, "no single-pass register kernel for one of the lengths");
  for (int nb_ : {in_blocks, out_blocks})
    if (!is_pow2(nb_) || nb_ > max_split_blocks(n1) || n1 % nb_) return fail(GFFT_ERR_UNSUPPORTED, "block count not supported for this length");
  if ((double)np * (double)n1 >= 2147483648.0 || (double)np * (double)n2 >= 2147483648.0) return fail(GFFT_ERR_UNSUPPORTED, "batch exceeds 2^31");
  const int64_t esz = 2 * (int64_t)precision;
  auto pl = new_plan(0, kind, precision);
  bool fused = false;
  rc = build_pair2d(pl.get(), cols, n2, planes, kind == GFFT_C2C_BACKWARD, cols_first, in_blocks, in_block_stride, out_blocks, out_block_stride, false, &fused);
  if (rc) return rc;
  pl->passes.back().carries_scale = true;
  const double elems = (double)np * (double)n1 * (double)n2;
  pl->flops = 5.0 * elems * std::log2((double)n1 * (double)n2);
  pl->bytes = 4.0 * elems * (double)esz;
  return publish(plan, std::move(pl));
}

/* The two local stages of a REAL slab-decomposed transform as one plan (see include/gfft.h). */
int gfft_plan_create_guru2_real(gfft_plan *plan, int precision, int kind, const gfft_iodim *cols, const gfft_iodim *rows,
                                const gfft_iodim *planes, int in_blocks, int64_t in_block_stride, int out_blocks,
                                int64_t out_block_stride) {
  if (!plan || !cols || !rows || !planes) return fail(GFFT_ERR_INVALID, "null argument");
  *plan = nullptr;
  if (int bad = check_precision(precision)) return bad;
  if (kind != GFFT_R2C && kind != GFFT_C2R) return fail(GFFT_ERR_UNSUPPORTED, "guru2_real plans are r2c / c2r (complex pairs: gfft_plan_create_guru2)");
  const bool inverse = kind == GFFT_C2R;
  const int64_t n1 = cols->n, n2 = rows->n, np = planes->n;
  if (n1 < 1 || n2 < 1 || np < 1) return fail(GFFT_ERR_INVALID, "bad length");
  if (rows->is != 1 || rows->os != 1) return fail(GFFT_ERR_UNSUPPORTED, "the row axis must be contiguous on both sides");
  if (cols->is < 1 || cols->os < 1 || planes->is < 1 || planes->os < 1) return fail(GFFT_ERR_INVALID, "strides must be positive");
  if (in_blocks < 1 || out_blocks < 1) return fail(GFFT_ERR_INVALID, "bad block count");
  if ((inverse ? out_blocks : in_blocks) > 1) return fail(GFFT_ERR_INVALID, "blocks on the half-spectrum side only (R2C: output, C2R: input)");
  // the two sides in their own elements: reals on the real side, complex entries on the half-spectrum side
  const int64_t H = n2 / 2 + 1;
  const int64_t re_es = inverse ? cols->os : cols->is, re_plane = inverse ? planes->os : planes->is;
  const int64_t cx_es = inverse ? cols->is : cols->os, cx_plane = inverse ? planes->is : planes->os;
  const int nb = inverse ? in_blocks : out_blocks;
  const int64_t bstride = inverse ? in_block_stride : out_block_stride;
  if (re_es < n2 || cx_es < H) return fail(GFFT_ERR_INVALID, "rows of a plane overlap (row stride below the row's length)");
  if (nb > 1 && n1 % nb == 0 && bstride < (n1 / nb) * cx_es) return fail(GFFT_ERR_INVALID, "block stride smaller than the block's extent");
  int rc = check_device();
  if (rc) return rc;
  if (n2 % 2 || n2 / 2 > 4096 || !real_half_supported((int)(n2 / 2)) || !regk_ok(n1, precision) || mixv_supported((int)n1))
    return fail(GFFT_ERR_UNSUPPORTED, "no single-pass register kernel for one of the lengths");
  if (!is_pow2(nb) || nb > max_split_blocks(n1) || n1 % nb) return fail(GFFT_ERR_UNSUPPORTED, "block count not supported for this length");
  if (re_es % 2 || re_plane % 2) return fail(GFFT_ERR_UNSUPPORTED, "real-side strides must be even (rows are read as complex pairs)");
  if ((double)np * (double)n1 >= 2147483648.0 || (double)np * (double)H >= 2147483648.0) return fail(GFFT_ERR_UNSUPPORTED, "batch exceeds 2^31");
  auto pl = new_plan(0, kind, precision);
  rc = build_pair2d_real(pl.get(), n1, n2, np, re_es, re_plane, cx_es, cx_plane, nb, bstride, inverse);
  if (rc) return rc;
  return publish(plan, std::move(pl));
}

/* Tile-major layouts of exchange buffers (see include/gfft.h). */
int gfft_plan_set_tiles(gfft_plan pl, int side, int tile, int64_t tile_stride) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (side != 0 && side != 1) return fail(GFFT_ERR_INVALID, "side must be 0 (input) or 1 (output)");
  if (pl->passes.size() != 1 || pl->fused3) return fail(GFFT_ERR_UNSUPPORTED, "tile-major layouts: single-pass plans only");
  Pass &p = pl->passes[0];
  if (p.kind != PK_FFT || !p.regk || p.d.mode != MODE_C2C || p.d.tw_hi || p.d.tr_dir || mixv_supported(p.d.n))
    return fail(GFFT_ERR_UNSUPPORTED, "tile-major layouts: plain complex register-kernel passes only");
  const int lg = ilog2_ceil(tile);
  if (tile < 0 || (tile > 0 && (!is_pow2(tile) || tile < 2 || tile_stride < tile)))
    return fail(GFFT_ERR_INVALID, "tile must be a power of two >= 2 (0 switches the layout off)");
  PassDesc &d = p.d;
  if (p.cols) {
    // the adjacent columns (innermost batch dim) are tile-major
    if (side == 0) { d.in_ilg = tile ? lg : 0; d.in_iS = tile ? tile_stride : 0; }
    else { d.out_ilg = tile ? lg : 0; d.out_iS = tile ? tile_stride : 0; }
    return GFFT_OK;
  }
  // ROWS: the transformed axis itself is tile-major; thread slots advance by NT entries, which must be
  // whole tiles, and blocks must be whole tiles too
  const int64_t n = d.n;
  const int nb = p.blocks[side];
  if (tile) {
    const int nt = pow2_rows_nt(n, pl->precision);
    if (!nt || nt % tile || (n / nb) % tile)
      return fail(GFFT_ERR_UNSUPPORTED, "tile-major rows: the line's thread layout does not advance by whole tiles");
  }
  const int64_t es = 1;
  const int64_t per = n / nb;
  const int64_t span = tile ? (per / tile) * tile_stride : per * es;     // what one block advances the address by
  const int64_t jump = nb > 1 ? p.bstride[side] - span : 0;
  if (side == 0) { d.in_tlg = tile ? lg : 0; d.in_tS = tile ? tile_stride : 0; d.in_jump = jump; }
  else { d.out_tlg = tile ? lg : 0; d.out_tS = tile ? tile_stride : 0; d.out_jump = jump; }
  return GFFT_OK;
}

int gfft_plan_set_flat(gfft_plan pl, int64_t body_width, int64_t tail_offset, int64_t tail_row_stride) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (pl->passes.size() != 1 || pl->fused3) return fail(GFFT_ERR_UNSUPPORTED, "flat tiles: single-pass plans only");
  Pass &p = pl->passes[0];
  if (p.kind != PK_FFT || !p.regk || !p.cols || p.d.mode != MODE_C2C || p.d.tw_hi || p.d.tr_dir)
    return fail(GFFT_ERR_UNSUPPORTED, "flat tiles: plain complex strided register-kernel passes only");
  if (body_width < 0 || body_width > p.d.inner) return fail(GFFT_ERR_INVALID, "body width must lie in 0 .. columns per row");
  p.d.flat = 1;
  p.d.fl_bw = (body_width > 0 && body_width < p.d.inner) ? body_width : 0;
  p.d.fl_tail = tail_offset;
  p.d.fl_tail_ms = tail_row_stride;
  return GFFT_OK;
}

int gfft_plan_set_split_slabs(gfft_plan pl, int side, int nblocks, int64_t rows_per_slab, int tile) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (pl->passes.size() != 1 || pl->axes.size() != 1 || pl->fused3)
    return fail(GFFT_ERR_UNSUPPORTED, "split layouts fuse into single-pass plans only");
  Pass &p = pl->passes[0];
  if (!((p.d.mode == MODE_R2C_H && side == 1) || (p.d.mode == MODE_C2R_H && side == 0)))
    return fail(GFFT_ERR_UNSUPPORTED, "slab-wise split: the half-spectrum side of packed-real rows only");
  // Every failure below leaves the plan as it was; a repeated call starts from the natural row strides again (the
  // slab form multiplies them), and one block switches the slab form off altogether.
  const PassDesc saved = p.d;
  auto bail = [&](int code, const char *msg) { p.d = saved; return fail(code, msg); };
  if (p.d.ub_n1 > 0) {
    p.d.inner = 1;
    p.d.in_os = p.d.in_is;   p.d.in_is = 1;
    p.d.out_os = p.d.out_is; p.d.out_is = 1;
    p.d.ub_n1 = 0;
    p.d.ub_tlg = 0;
  }
  if (p.d.tr_dir || p.d.mid != 1 || p.d.inner != 1) return bail(GFFT_ERR_UNSUPPORTED, "slab-wise split: plain packed-real rows only");
  const int lg = ilog2_ceil(tile);
  if (tile < 2 || !is_pow2(tile)) return bail(GFFT_ERR_INVALID, "tile must be a power of two >= 2");
  if (rows_per_slab < 1 || p.d.batch % rows_per_slab) return bail(GFFT_ERR_INVALID, "rows per slab must divide the number of rows");
  // (the kernels address this layout with 32-bit element offsets)
  if ((double)p.d.batch * ((double)p.d.n + 1.0) >= 2147483648.0) return bail(GFFT_ERR_UNSUPPORTED, "slab-wise split: buffer beyond 2^31 entries");
  int rc = gfft_plan_set_split(pl, side, nblocks);
  if (rc) { p.d = saved; return rc; }
  if (nblocks == 1) return GFFT_OK;
  PassDesc &d = p.d;
  // rows of the batch as (slab, row in slab): the kernel's (o, i) indices
  d.inner = rows_per_slab;
  d.in_is = d.in_os;   d.in_os *= rows_per_slab;
  d.out_is = d.out_os; d.out_os *= rows_per_slab;
  d.ub_n1 = rows_per_slab;
  d.ub_tlg = lg;
  for (int b = 0; b < 8; ++b) d.ub_base[b] = b < nblocks ? d.ub_rows * (int64_t)d.ub_start[b] : 0;
  return GFFT_OK;
}

/* free the shared scratch buffers (they are otherwise kept for the life of the process) */
int gfft_scratch_release(void) { return scratch_pool().release(true); }

/* Did a fused launch of ANY plan give up a wait since the last look?  GFFT_OK, or GFFT_ERR_VOIDED once per event with the plan
 * named in gfft_last_error().  Does not synchronise: call it after the stream (or device) has been synchronised to learn
 * whether the results that synchronisation waited for are valid (include/gfft.h). */
int gfft_async_error(void) { return poll_async_error(nullptr); }
int gfft_plan_status(gfft_plan pl) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  return poll_async_error(pl);
}

int gfft_plan_destroy(gfft_plan pl) {
  if (!pl) return GFFT_OK;
  std::unique_ptr<gfft_plan_s>(pl).reset();      // the one place a published plan dies (publish() handed it to the caller)
  if (--g_live_plans == 0) (void)scratch_pool().release(false);
  return GFFT_OK;
}

int gfft_plan_describe(gfft_plan pl, char *buf, size_t len) {
  if (!pl || !buf || !len) return fail(GFFT_ERR_INVALID, "null argument");
  std::string s;
  char line[256];
  const char *kn = pl->kind == GFFT_C2C_FORWARD ? "c2c-forward" : pl->kind == GFFT_C2C_BACKWARD ? "c2c-backward"
                   : pl->kind == GFFT_R2C ? "r2c" : "c2r";
  char sched[96] = "";
  if (pl->fused3 && pl->ws_tile) snprintf(sched, sizeof sched, " [3-D schedule: tile-major workspace, tiles of %d columns]", pl->ws_tile);
  else if (pl->fused3) snprintf(sched, sizeof sched, " [3-D schedule: padded-pitch workspace, rows %lld entries apart]", (long long)pl->ws_pitch);
  snprintf(line, sizeof line, "gfft plan: %s %s, %d dims, %zu passes%s\n", kn, pl->precision == 8 ? "f64" : "f32",
           pl->ndims, pl->passes.size(), sched);
  s += line;
  static const char *bufn[] = {"IN", "OUT", "WS", "FS", "AUX", "RING", "FS2"};
  for (const Pass &p : pl->passes) {
    if (p.kind == PK_FUSED2) {
      const char *fk = kFusedKinds[p.fused_kind].describe_name;
      if (pl->fused_off)
        snprintf(line, sizeof line, "  pair (%s) n=%d then n=%d as two stand-alone passes (a fused launch gave up a wait)%s  %s -> %s\n",
                 fk, p.d.n, p.d2.n, p.carries_scale ? " [scale]" : "", bufn[p.src], bufn[p.dst]);
      else
      snprintf(line, sizeof line, "  fused pair (%s) n=%d then n=%d: %d planes, %d + %d tiles per plane, ring of %d slots x %lld KiB, one persistent launch%s  %s -> %s\n",
               fk, p.d.n, p.d2.n, p.fused.planes, p.fused.tiles_a, p.fused.tiles_b, p.fused.ring,
               (long long)(p.fused.slot_bytes >> 10), p.carries_scale ? " [scale]" : "", bufn[p.src], bufn[p.dst]);
      s += line;
      continue;
    }
    if (p.kind == PK_PLANE2D) {
      snprintf(line, sizeof line, "  planes on chip: rows n=%d then columns n=%d of %d planes held in LDS, one launch%s  %s -> %s\n", p.d.n, p.d2.n,
               p.fused.planes, p.carries_scale ? " [scale]" : "", bufn[p.src], bufn[p.dst]);
      s += line;
      continue;
    }
    if (p.kind != PK_FFT) {
      static const char *kinds[] = {"", "embed (chirp/zero-pad into AUX)", "multiply by B = FFT(chirp)", "extract (chirp, scale)"};
      snprintf(line, sizeof line, "  %s n=%lld Lw=%lld  %s -> %s\n", kinds[p.kind], (long long)p.pt.n,
               (long long)p.pt.Lw, bufn[p.src], bufn[p.dst]);
      s += line;
      continue;
    }
    snprintf(line, sizeof line, "  n=%d batch=%lld (mid=%lld inner=%lld) es_in=%lld es_out=%lld kernel=%s%s%s  %s -> %s\n",
             p.d.n, (long long)p.d.batch, (long long)p.d.mid, (long long)p.d.inner, (long long)p.d.in_es,
             (long long)p.d.out_es,
             (p.d.mode == MODE_R2C_H || p.d.mode == MODE_C2R_H) ? "regs-rows packed-real (n = complex length)"
             : p.regk ? (p.cols ? "regs-cols" : "regs-rows") : "generic",
             p.d.tw_hi ? " [four-step 1/2, fused twiddle]" : "", p.carries_scale ? " [scale]" : "",
             bufn[p.src], bufn[p.dst]);
    s += line;
  }
  snprintf(buf, len, "%s", s.c_str());
  return GFFT_OK;
}

int gfft_plan_cost(gfft_plan pl, double *flops, double *bytes, int *launches) {
  if (!pl) return fail(GFFT_ERR_INVALID, "null plan");
  if (flops) *flops = pl->flops;
  if (bytes) *bytes = pl->bytes;
  if (launches) *launches = (int)pl->passes.size();
  return GFFT_OK;
}

// the data-movement kernels address whole items: both arrays aligned as one (include/gfft.h)
static int check_items(const void *a, const void *b, int itemsize) {
  if (itemsize != 4 && itemsize != 8 && itemsize != 16) return fail(GFFT_ERR_INVALID, "itemsize must be 4, 8 or 16");
  if (((uintptr_t)a | (uintptr_t)b) % (uintptr_t)itemsize)
    return fail(GFFT_ERR_INVALID, "arrays must be aligned to " + std::to_string(itemsize) + " bytes (one element)");
  return GFFT_OK;
}

static int collapse(int ndims, const int64_t *shape, int axis, int64_t *outer, int64_t *naxis, int64_t *inner) {
  if (!shape || ndims < 1 || axis < 0 || axis >= ndims) return fail(GFFT_ERR_INVALID, "bad shape/axis");
  *outer = *inner = 1;
  for (int i = 0; i < axis; ++i) *outer *= shape[i];
  for (int i = axis + 1; i < ndims; ++i) *inner *= shape[i];
  *naxis = shape[axis];
  return GFFT_OK;
}

int gfft_pack(const void *d_array, void *d_packed, int ndims, const int64_t *shape, int axis, int nparts,
              int itemsize, void *stream) {
  int64_t o, n, i;
  int rc = collapse(ndims, shape, axis, &o, &n, &i);
  if (rc) return rc;
  if (nparts < 1 || n < nparts) return fail(GFFT_ERR_INVALID, "axis shorter than the number of parts");
  if ((rc = check_items(d_array, d_packed, itemsize))) return rc;
  if ((rc = check_device())) return rc;
  HIP_TRY(launch_pack(d_array, d_packed, o, n, i, nparts, itemsize, false, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_unpack(const void *d_packed, void *d_array, int ndims, const int64_t *shape, int axis, int nparts,
                int itemsize, void *stream) {
  int64_t o, n, i;
  int rc = collapse(ndims, shape, axis, &o, &n, &i);
  if (rc) return rc;
  if (nparts < 1 || n < nparts) return fail(GFFT_ERR_INVALID, "axis shorter than the number of parts");
  if ((rc = check_items(d_packed, d_array, itemsize))) return rc;
  if ((rc = check_device())) return rc;
  HIP_TRY(launch_pack(d_packed, d_array, o, n, i, nparts, itemsize, true, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_truncate(const void *d_padded, void *d_trunc, int ndims, const int64_t *shape_padded, int axis,
                  int64_t n_trunc, int is_real, int precision, double scale, void *stream) {
  int64_t o, n, i;
  int rc = collapse(ndims, shape_padded, axis, &o, &n, &i);
  if (rc) return rc;
  if (n_trunc < 1 || n_trunc > n) return fail(GFFT_ERR_INVALID, "bad truncated length");
  if ((rc = check_precision(precision)) || (rc = check_items(d_padded, d_trunc, 2 * precision))) return rc;
  if ((rc = check_device())) return rc;
  HIP_TRY(launch_trunc(d_padded, d_trunc, o, n, n_trunc, i, is_real, precision, scale, false, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_pad(const void *d_trunc, void *d_padded, int ndims, const int64_t *shape_padded, int axis,
             int64_t n_trunc, int is_real, int precision, void *stream) {
  int64_t o, n, i;
  int rc = collapse(ndims, shape_padded, axis, &o, &n, &i);
  if (rc) return rc;
  if (n_trunc < 1 || n_trunc > n) return fail(GFFT_ERR_INVALID, "bad truncated length");
  if ((rc = check_precision(precision)) || (rc = check_items(d_trunc, d_padded, 2 * precision))) return rc;
  if ((rc = check_device())) return rc;
  HIP_TRY(launch_trunc(d_trunc, d_padded, o, n, n_trunc, i, is_real, precision, 1.0, true, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_scale(void *d_data, int64_t count, int precision, double scale, void *stream) {
  int rc = check_precision(precision);
  if (rc || (rc = check_items(d_data, d_data, precision))) return rc;
  if ((rc = check_device())) return rc;
  HIP_TRY(launch_scale(d_data, count, precision, scale, (hipStream_t)stream));
  return GFFT_OK;
}

int gfft_malloc(void **d_ptr, size_t bytes) {
  int rc = check_device();
  if (rc) return rc;
  hipError_t e = hipMalloc(d_ptr, bytes);
  if (e == hipErrorOutOfMemory) return fail(GFFT_ERR_NOMEM, "hipMalloc: out of memory");
  HIP_TRY(e);
  return GFFT_OK;
}
int gfft_free(void *d_ptr) { HIP_TRY(hipFree(d_ptr)); return GFFT_OK; }
int gfft_memcpy_h2d(void *d, const void *h, size_t n, void *s) { HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, (hipStream_t)s)); return GFFT_OK; }
int gfft_memcpy_d2h(void *h, const void *d, size_t n, void *s) { HIP_TRY(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, (hipStream_t)s)); return GFFT_OK; }
int gfft_memcpy_d2d(void *d, const void *s_, size_t n, void *s) { HIP_TRY(hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToDevice, (hipStream_t)s)); return GFFT_OK; }
int gfft_stream_synchronize(void *s) { HIP_TRY(hipStreamSynchronize((hipStream_t)s)); return GFFT_OK; }

int gfft_event_create(void **event) {
  int rc = check_device();
  if (rc) return rc;
  hipEvent_t e;
  HIP_TRY(hipEventCreate(&e));
  *event = e;
  return GFFT_OK;
}
int gfft_event_record(void *event, void *stream) { HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream)); return GFFT_OK; }
int gfft_event_elapsed_ms(void *start, void *stop, float *ms) {
  HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return GFFT_OK;
}
int gfft_event_destroy(void *event) { HIP_TRY(hipEventDestroy((hipEvent_t)event)); return GFFT_OK; }

/* developer probe: run ONE power-of-two pass with explicit batch geometry and strides
 * (element units), bypassing the planner.  geom = {n, outer, mid, inner, in_os, in_ms, in_is,
 * in_es, out_os, out_ms, out_is, out_es}.  Not part of the drop-in boundary. */
int gfft_debug_pass(const int64_t *geom, int precision, int cols, int variant, int inverse,
                    const void *d_in, void *d_out, void *stream) {
  int rc = check_device();
  if (rc) return rc;
  PassDesc d{};
  d.n = (int)geom[0];
  d.mode = MODE_C2C;
  d.conj_in = d.conj_out = inverse;
  d.mid = geom[2];
  d.inner = geom[3];
  d.batch = geom[1] * geom[2] * geom[3];
  d.in_os = geom[4]; d.in_ms = geom[5]; d.in_is = geom[6]; d.in_es = geom[7];
  d.out_os = geom[8]; d.out_ms = geom[9]; d.out_is = geom[10]; d.out_es = geom[11];
  d.scale = 1.0;
  d.flat = opts().debug_flat;
  d.swizzle = opts().xcd_swizzle > 0 ? 1 : 0;
  if (!cols && (opts().debug_tile_side & 1)) { d.in_tlg = opts().debug_tile_lg; d.in_tS = opts().debug_tile_stride; }
  if (!cols && (opts().debug_tile_side & 2)) { d.out_tlg = opts().debug_tile_lg; d.out_tS = opts().debug_tile_stride; }
  rc = get_twiddles(d.n, precision, &d.tw);
  if (rc) return rc;
  hipError_t e = precision == 8 ? launch_pow2_f64(d, cols != 0, variant, d_in, d_out, (hipStream_t)stream)
                                : launch_pow2_f32(d, cols != 0, variant, d_in, d_out, (hipStream_t)stream);
  HIP_TRY(e);
  return GFFT_OK;
}

int gfft_probe_copy(const void *d_src, void *d_dst, size_t bytes, void *stream) {
  int rc = check_device();
  if (rc) return rc;
  HIP_TRY(launch_copy(d_src, d_dst, bytes, (hipStream_t)stream));
  return GFFT_OK;
}
int gfft_probe_tile_copy(const void *d_src, void *d_dst, int64_t outer, int64_t n, int64_t inner, int tcols, void *stream) {
  int rc = check_device();
  if (rc) return rc;
  HIP_TRY(launch_tile_copy(d_src, d_dst, outer, n, inner, tcols, (hipStream_t)stream));
  return GFFT_OK;
}

}  // extern "C"
