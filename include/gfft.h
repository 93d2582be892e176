/* gfft.h -- C ABI of libgfft.so, the MI355X (gfx950) engine behind the PFFT hot path.
 *
 * Drop-in boundary: these entry points are what mpi4py-fft's native layer binds today
 * (Cython `fftw_xfftn.FFT` over `fftw_planxfftn`, plus what MPI's datatype engine does inside
 * `Alltoallw`), re-expressed for device memory:
 *
 *   gfft_plan_create    <- fftw_planxfftn()            mpi4py_fft/fftw/fftw_planxfftn.h:9-17, .c:10-77
 *   gfft_execute        <- fftw_execute_dft{,_r2c,_c2r}  mpi4py_fft/fftw/fftw_xfftn.pyx:29-48,291-292
 *   gfft_plan_destroy   <- fftw_destroy_plan()         mpi4py_fft/fftw/fftw_xfftn.pyx:162-163
 *   gfft_plan_describe  <- fftw_print_plan()           mpi4py_fft/fftw/fftw_xfftn.pyx:173-175
 *   gfft_pack/unpack    <- Create_subarray + Alltoallw's pack/unpack   mpi4py_fft/pencil.py:12-29,182,200
 *   gfft_truncate/pad   <- FFTBase._truncation_forward/_padding_backward  mpi4py_fft/libfft.py:263-311
 *   gfft_scale          <- `output_array *= M`         mpi4py_fft/libfft.py:412-413, fftw_xfftn.pyx:293-294
 *
 * Conventions: every function returns 0 (GFFT_OK) or a negative gfft_status; nothing throws
 * across the ABI.  All pointers named d_* are DEVICE pointers, borrowed (never owned or freed by
 * the library).  All work is enqueued asynchronously on `stream` (a hipStream_t passed as void*;
 * NULL = the default stream).  Sizes and strides are 64-bit (the reference's C planner uses
 * `int`, fftw_planxfftn.c:11-22; 1024^3 is its edge).  Arrays are C-contiguous (row-major), the
 * only layout the reference plans for (fftw_planxfftn.c:25-30).  Caller is single-threaded per
 * plan.  No host fallback exists: without a HIP device every compute entry point returns
 * GFFT_ERR_NO_DEVICE.
 *
 * Scratch and re-entrancy: plans that need a workspace (3-D all-axes plans, multi-axis c2r, four-step
 * and Bluestein lengths) carve it from ONE buffer per (calling thread, stream), shared by every
 * plan that thread executes on that stream and grown -- with a synchronisation of that stream --
 * when a larger request arrives (gfft_scratch_release frees them; so does destroying the last
 * plan of the process).  Consequences: (1) a thread may
 * run any sequence of plans on a stream; (2) two executions issued by one thread that may overlap
 * in time must be on different streams; (3) the first
 * gfft_execute of the largest plan on a stream allocates, so run each plan once on the stream
 * before capturing it into a HIP graph -- after that gfft_execute and the pointwise entries only
 * enqueue kernels (no allocation, no synchronisation); (4) a workspace handed out during a capture is
 * baked into the graph, so the library pins it: neither a larger plan arriving later nor the last plan
 * being destroyed frees it -- only gfft_scratch_release() does, and the caller must not replay such a
 * graph after calling it.
 */
#ifndef GFFT_H
#define GFFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gfft_plan_s *gfft_plan;

typedef enum {
  GFFT_OK = 0,
  GFFT_ERR_INVALID = -1,     /* bad argument (shape/axes/kind mismatch)                */
  GFFT_ERR_UNSUPPORTED = -2, /* valid request the engine cannot plan (e.g. huge prime) */
  GFFT_ERR_NO_DEVICE = -3,   /* no HIP device / HIP runtime failure at init            */
  GFFT_ERR_HIP = -4,         /* a HIP call failed; see gfft_last_error()               */
  GFFT_ERR_NOMEM = -5,
  GFFT_ERR_VOIDED = -6       /* a launch that had already returned GFFT_OK failed on the device: gfft_async_error() */
} gfft_status;

/* transform kinds: same integers as the reference (fftw_planxfftn.c:3-8, utilities.pyx:7-26) */
enum { GFFT_C2C_FORWARD = -1, GFFT_C2C_BACKWARD = +1, GFFT_R2C = -2, GFFT_C2R = +2 };
/* real-to-real kinds: the integers of FFTW's fftw_r2r_kind as utilities.pyx:7-20 exposes them */
enum { GFFT_REDFT00 = 3, GFFT_REDFT01 = 4, GFFT_REDFT10 = 5, GFFT_REDFT11 = 6,
       GFFT_RODFT00 = 7, GFFT_RODFT01 = 8, GFFT_RODFT10 = 9, GFFT_RODFT11 = 10, GFFT_R2R = 100 };
/* precision of the real type: float (fftwf_* clone, setup.py:93-111) or double */
enum { GFFT_F32 = 4, GFFT_F64 = 8 };

const char *gfft_strerror(int status);
const char *gfft_last_error(void);          /* detail of the last failure on this thread */
int gfft_version(void);
int gfft_device_count(int *count);          /* hipGetDeviceCount; GFFT_ERR_NO_DEVICE if none */
int gfft_device_name(int device, char *buf, size_t len);
/* tunables consulted when a plan is created: "grid_cap" (> 0: workgroups per launch at most, for every pass kernel whose
 * workgroups walk their tiles -- the register kernels, the generic and per-column kernels, the on-chip planes, the Bluestein
 * point kernels; set it before the plan is made and keep it through the executes; 0: each launcher's own cap; persistent fused
 * pairs and the pack / truncate / scale kernels do not look at it; gfft_plan_pass_launch reports the outcome), "variant_rows",
 * "variant_cols", "force_generic", "fused3", "profile" (also readable from the environment as GFFT_<UPPERCASE NAME>);
 * "fuse2" (1: pass pairs as one persistent launch through the Infinity Cache where a pair exists and pays,
 * 0: stand-alone passes), with "fuse2_ring" / "fuse2_lag" (slots of the hand-off ring /
 * planes the producer runs ahead; 0 = auto: about 96 MiB of lead and twice that of ring -- 12 / 6 planes of 16 MiB, 24 / 12 of
 * 8 MiB, 48 / 24 of 4 MiB --, launches with too few planes for that stay unfused), "fuse2_kinds" (bit mask of pair kinds:
 * 2 strided->rows, 4 / 16 four-step, 8 batched 2-D, 32 r2c rows->strided, 64 strided->c2r rows, 128 / 256 the complex slab
 * pairs of gfft_plan_create_guru2 with blocks, 512 / 1024 the real slab pairs of gfft_plan_create_guru2_real; default 2046 = all
 * but bit 1, [rows->strided] of the one-rank 3-D schedule), "fuse2_f32" (1: complex64
 * pairs, 2: real fp32 pairs too), "fuse2_n512" (the n = 512 pairs: 0 off, 1 on 16 lines per tile, 2 [strided -> rows] on 32), "fuse2_mixed" (pairs on planes of 512 x 1024 / 1024 x 512 points), "fuse2_f32_n512" (the complex64 n = 512 pairs), "fuse2_wait_ms" (wall-clock limit of a wait inside a fused
 * launch before the launch voids itself, gfft_async_error below; default 2000); GFFT_FUSE2_DEBUG=1 prints a fused
 * launch's counters.  ("debug_tw_index" / "debug_tw_exp": TEST HOOK -- twiddle tables uploaded while debug_tw_exp > 0
 * carry one entry off by 10^-debug_tw_exp: what the rounding-level guards of tests/ must catch; "debug_tw_len" != 0 confines
 * it to tables of exactly that length -- a packed-real plan's Hermitian table rtw(n) and not its tw(n / 2).
 * "debug_r2r_index" / "debug_r2r_exp" / "debug_r2r_post": the same TEST HOOK for the pre (0) / post (1) tables of the
 * real-to-real kinds.) */
int gfft_set_option(const char *key, int value);

/* ---- serial multi-axis transform plan ------------------------------------------------
 * Same decomposition as fftw_planxfftn(): transform dims = `axes` (executed last-listed axis
 * first; for R2C/C2R the halved axis is axes[naxes-1], xfftn.py:231-232,309-315), every other
 * dim is a batch dim.  sizes_in/sizes_out are the full array shapes (they differ only along
 * axes[naxes-1] for R2C/C2R: n vs n/2+1).  R2C/C2R logical length n is taken from the real
 * side, as fftw_planxfftn.c:23 does.  */
int gfft_plan_create(gfft_plan *plan, int ndims, const int64_t *sizes_in, const int64_t *sizes_out,
                     int naxes, const int *axes, int kind, int precision);
/* Real-to-real plan: the `default:` branch of fftw_planxfftn (fftw_planxfftn.c:68-75,
 * fftw_plan_guru_r2r).  One kind per transformed axis (GFFT_REDFT00 .. GFFT_RODFT11 = DCT-I,
 * DCT-III, DCT-II, DCT-IV, DST-I, DST-III, DST-II, DST-IV in FFTW's unnormalised definitions);
 * input and output are real arrays of shape `sizes`; in-place execution is allowed. */
int gfft_plan_create_r2r(gfft_plan *plan, int ndims, const int64_t *sizes, int naxes, const int *axes,
                         const int *kinds, int precision);
/* out = scale * DFT(in).  d_in == d_out is allowed for C2C and real-to-real plans.  Every
 * out-of-place execution PRESERVES its input -- part of the contract: multi-axis C2R (where FFTW
 * destroys the input) routes its complex passes through the workspace, and the Python host relies
 * on it when it reads a caller's array in place (Transform.__call__).
 * Footprint: an execution reads nothing outside the plan's input array that any output depends on and writes
 * nothing outside its output array (and the library's own workspace): tests/test_gpu_guard_*.py hold both.
 * Base alignment: d_in and d_out must each be aligned as ONE ELEMENT of their array -- `precision` bytes for a
 * real array, 2 * precision for a complex one -- and need no more: a view that starts at any element of a larger
 * allocation is a valid argument and gives the bits of an aligned one.  (Every kernel addresses its arrays
 * element by element; the compiler widens accesses only where the hardware takes them at any alignment.)  One
 * exception: a REAL plan that runs a fused pass pair (gfft_plan_create_guru2_real where it has fused kernels; the
 * [r2c rows -> strided] / [strided -> c2r rows] pairs of a multi-axis gfft_plan_create plan, option fuse2_kinds
 * bits 32 / 64) streams its real side as complex pairs: that side must be aligned to 2 * precision bytes, whether
 * or not the pair is still fused.  GFFT_ERR_INVALID, with the requirement in gfft_last_error(), otherwise; nothing
 * is enqueued.
 * In place (d_in == d_out): real r2c / c2r plans refuse it.  So does a complex plan whose two sides are laid out
 * differently -- one side re-laid-out by gfft_plan_set_split / gfft_plan_set_tiles / gfft_plan_set_flat with a body
 * width, blocks on one side of a guru plan, a fused truncation / zero padding (gfft_plan_set_truncation,
 * gfft_plan_create_guru_padded) --: a workgroup loads a whole tile before it stores it, which makes in-place
 * execution safe exactly when every tile writes the addresses it read.  GFFT_ERR_INVALID; nothing is enqueued. */
int gfft_execute(gfft_plan plan, const void *d_in, void *d_out, double scale, void *stream);
int gfft_plan_destroy(gfft_plan plan);
int gfft_scratch_release(void);           /* frees the shared per-stream workspaces, pinned ones included */
/* Errors of launches that have already returned GFFT_OK (execution is asynchronous): a fused pass-pair launch
 * whose workgroups waited longer than option "fuse2_wait_ms" (default 2000) for one another -- a device shared
 * with a long foreign kernel, a debugger -- voids itself instead of hanging or trapping.  The results of that plan's
 * last execution are invalid and the plan runs the pair as stand-alone launches from then on.  The event stays with
 * ITS plan until it is reported once, as GFFT_ERR_VOIDED with the plan named in gfft_last_error(), by whichever of
 * these looks first:
 *   gfft_plan_status(plan)  this plan's pending event;
 *   gfft_execute(plan, ..)  the same, before enqueueing anything (other plans' events do not refuse the call);
 *   gfft_async_error()      any plan's pending event (call until GFFT_OK to drain several).
 * None of them synchronises -- call after synchronising the stream to learn whether what was waited for is valid.
 * (The reference raises RuntimeError where FFTW fails to plan, mpi4py_fft/fftw/fftw_xfftn.pyx:152-153, and cannot
 * fail afterwards; this is the analogue for a failure mode only a persistent launch has.) */
int gfft_async_error(void);
int gfft_plan_status(gfft_plan plan);
/* Fuse FFTBase._truncation_forward / _padding_backward (libfft.py:263-311) into a single-axis plan:
 * afterwards gfft_execute writes (forward kinds) / reads (backward kinds) the TRUNCATED array,
 * n_keep entries along the axis (N on a complex axis, N/2+1 on the real half-axis), with the
 * reference's Nyquist rules.  GFFT_ERR_UNSUPPORTED = not fusable for this plan (use
 * gfft_truncate / gfft_pad); the plan is left unchanged. */
int gfft_plan_set_truncation(gfft_plan plan, int64_t n_keep);
/* The whole padded 3-D transform of a one-rank PFFT(padding=...) as ONE plan: what the reference runs
 * as three FFT objects, each followed (forward) by _truncation_forward or preceded (backward) by
 * _padding_backward (libfft.py:263-311, 408-422; chained by mpifft.py:68-73 with identity transfers).
 * `padded` = the transformed lengths = shape of the physical array (real for R2C / C2R); `kept` =
 * shape of the truncated spectral array (entries kept per axis: N on complex axes, N/2 + 1 on the
 * real half-axis, axis 2).  Forward kinds read the physical array and write the truncated one,
 * backward kinds the reverse; every pass carries its axis's truncating store / zero-padding load and
 * the intermediates live in the plan's pitched workspace (rows of the odd-width half spectrum start on
 * 128-byte lines there), never in arrays of the caller.  The input is preserved.
 * GFFT_ERR_UNSUPPORTED when a padded length has no single-pass kernel (caller keeps the per-axis
 * plans with gfft_plan_set_truncation). */
int gfft_plan_create_padded(gfft_plan *plan, const int64_t *padded, const int64_t *kept, int kind, int precision);
/* Fuse the pack / unpack side of Transfer (pencil.py:12-29,182,200: the subarray datatypes of
 * Alltoallw) into a single-axis complex plan.  side 1: gfft_execute writes its output directly
 * in the layout of the all-to-all SEND buffer for `nblocks` equal blocks of the transformed axis
 * -- what gfft_pack would produce from the natural output; side 0: it reads its input directly
 * from the RECEIVE buffer -- what gfft_unpack would consume.  nblocks = 1 restores the natural
 * layout.  GFFT_ERR_UNSUPPORTED (plan unchanged) when the plan is not one register-kernel pass or
 * nblocks is not a power of two <= 8 dividing the length.  Real transforms: the half-spectrum side
 * of an r2c (side 1) / c2r (side 0) plan along the contiguous last axis takes any nblocks <= 8 --
 * n/2 + 1 entries never split evenly, so the blocks follow the reference's block rule
 * (pencil.py:5-9) exactly as gfft_pack cuts them; other real plans return GFFT_ERR_UNSUPPORTED.
 * After gfft_plan_set_truncation the truncated side's blocks are blocks of the KEPT entries (complex
 * axes: equal blocks of a power of two of them; the real half-axis: the block rule over n_keep). */
int gfft_plan_set_split(gfft_plan plan, int side, int nblocks);
/* One batched 1-D complex transform with explicit strides: the form fftw_planxfftn() hands to
 * fftw_plan_guru_dft (fftw_planxfftn.c:25-57) -- `dim` is the transformed axis, `howmany` up to
 * three batch dims, slowest first; lengths and strides in elements, as fftw_iodim64 -- for callers
 * that run a stage of a distributed transform on sub-arrays and exchange buffers (the chunked,
 * stream-overlapped redistribution of mpi4py-fft_amd/pipeline.py).  Extension for exchange
 * buffers: the transformed axis may be stored as `in_blocks` / `out_blocks` equal blocks (a power
 * of two, 1 = contiguous) whose starts lie `*_block_stride` elements apart -- block b of the axis
 * is what rank b of the sub-communicator receives / sent.  kind: GFFT_C2C_FORWARD / _BACKWARD.
 * gfft_execute's d_in / d_out are the addresses of element 0.  GFFT_ERR_UNSUPPORTED when the
 * length has no single-pass register kernel or the block count does not fit its thread layout. */
typedef struct { int64_t n, is, os; } gfft_iodim;
int gfft_plan_create_guru(gfft_plan *plan, int precision, int kind, const gfft_iodim *dim, int howmany_rank,
                          const gfft_iodim *howmany, int in_blocks, int64_t in_block_stride, int out_blocks,
                          int64_t out_block_stride);
/* gfft_plan_create_guru with the 3/2-rule truncation (forward kind: on the store side) / zero padding
 * (backward kind: on the load side) of libfft.py:263-311 fused in, as gfft_plan_set_truncation fuses it
 * into natural plans: dim->n is the padded (transformed) length, `n_keep` the entries kept along the axis
 * on the truncated side -- the output of a forward plan, the input of a backward one -- whose stride
 * (dim->os / dim->is) and blocks then describe the TRUNCATED line: its blocks are equal blocks of the
 * kept entries (a power of two of them each), what the stage of a padded distributed transform
 * (mpifft.py:247-257 inflates the shape, :68-73 runs the chain) sends to / receives from its
 * sub-communicator.  n_keep = 0 or n: no truncation (= gfft_plan_create_guru). */
int gfft_plan_create_guru_padded(gfft_plan *plan, int precision, int kind, const gfft_iodim *dim, int64_t n_keep,
                                 int howmany_rank, const gfft_iodim *howmany, int in_blocks, int64_t in_block_stride,
                                 int out_blocks, int64_t out_block_stride);
/* The two LOCAL stages of a slab-decomposed transform as one plan.  The reference joins consecutive stages whose
 * redistribution stays on one rank with a whole-array self-Alltoallw (mpifft.py:324-331, pencil.py:168-183); the
 * staged form here elides that copy and runs two plans; this entry runs both transforms as ONE launch per
 * direction, plane by plane, the plane handed from the first pass to the second inside the Infinity Cache
 * (fft_pow2_impl.h fft_fused2_kernel) -- and the all-to-all buffer of the NEXT (previous) redistribution is
 * addressed by the strided pass itself, as gfft_plan_create_guru's blocks are.
 *   rows    the contiguous transformed axis (is = os = 1)
 *   cols    the strided transformed axis: n, is / os = distance between consecutive rows of a plane
 *   planes  the batch: n planes, is / os = distance between consecutive planes
 *   cols_first = 1: [cols, then rows] -- strided reads, whole rows written: the order the host uses in both directions
 *     (level with the other one in complex128, 9 % ahead in complex64: tools/stage_probe.py slab); 0: [rows, then cols].
 *   in_blocks / in_block_stride, out_blocks / out_block_stride: the cols axis stored as that many equal blocks whose
 *     starts lie that many elements apart (1 = contiguous) -- the receive buffer of the all-to-all that gathered that
 *     axis on the input side (backward direction), the send buffer of the one that scatters it on the output side
 *     (forward).  The strided pass adds the block jump to its step; the row pass places every row by its block.
 *     At most one side takes blocks.
 * kind: GFFT_C2C_FORWARD / _BACKWARD; gfft_execute's d_in / d_out are the addresses of element 0 and must not
 * overlap unless both sides have the same natural layout; the input is preserved otherwise.  Where the pair has
 * no fused kernels (planes other than 512 / 1024 points a side in fp64 -- equal or not --, 512 x 512 / 1024 x 1024 in fp32;
 * rows-first order outside the square fp64 / 1024 x 1024 fp32 pairs; too few planes for a hand-off ring) the
 * plan runs two stand-alone passes -- the first one carries the data across, the second works in place on the
 * output -- with the same results up to nothing: the arithmetic of a pass does not depend on its launch form.
 * GFFT_ERR_UNSUPPORTED when a length has no single-pass register kernel or the block count does not fit. */
int gfft_plan_create_guru2(gfft_plan *plan, int precision, int kind, const gfft_iodim *cols, const gfft_iodim *rows,
                           const gfft_iodim *planes, int cols_first, int in_blocks, int64_t in_block_stride,
                           int out_blocks, int64_t out_block_stride);
/* gfft_plan_create_guru2 for REAL input: the two local stages of a slab-decomposed r2c / c2r transform -- the reference's
 * default dtype (mpifft.py:202) -- as one plan, ONE launch per direction where a fused pair exists.
 *   kind = GFFT_R2C: [r2c rows, then cols] -- real planes in, half-spectrum planes (rows of n / 2 + 1 entries) out;
 *   kind = GFFT_C2R: [cols, then c2r rows] -- the mirror.  The order is fixed.
 *   rows    rows->n = the REAL length (even), contiguous on both sides (is = os = 1)
 *   cols    the strided axis: n, is / os = distance between consecutive rows of a plane
 *   planes  the batch: n planes, is / os = distance between consecutive planes
 *   Strides count elements of the side they describe: reals on the real side, complex entries on the half-spectrum side
 *   (real-side strides even: the rows are read / written as complex pairs, element 0 aligned as a pair).
 *   in_blocks / in_block_stride, out_blocks / out_block_stride: the cols axis stored as that many equal blocks whose starts lie
 *     that many complex entries apart -- allowed on the HALF-SPECTRUM side only (the output of R2C: the send buffer of the
 *     redistribution behind the stage pair; the input of C2R: the receive buffer in front of it).  1 = contiguous.
 * d_in and d_out must not overlap; the input is preserved.  GFFT_ERR_INVALID: non-positive strides, rows of a plane that
 * overlap, blocks on the real side, more than one block with a block stride below the block's extent (n / blocks rows).
 * GFFT_ERR_UNSUPPORTED: a length without a single-pass register kernel (rows: 32 ... 8192 reals, powers of two), a block
 * count that does not fit (a power of two up to 8 dividing cols->n), odd real-side strides, a complex kind.
 * Fused kernels (kinds FUSED_R2C_PLANES_B / FUSED_COLS_C2R_B, option bits 512 / 1024): fp64 with cols->n = 1024 and rows of
 * 1024 or 2048 reals (backward 2048: option c2r_2048, on by default), fp32 1024 x 1024 under option fuse2_f32 = 2; everywhere
 * else -- and after a fused launch gave up a wait -- the plan runs two stand-alone passes with the same results: forward r2c
 * rows IN -> OUT placed by block, then the strided pass in place on OUT; backward the strided pass IN -> plan workspace, then
 * the c2r rows -> OUT.  gfft_plan_cost's `launches` tells which. */
int gfft_plan_create_guru2_real(gfft_plan *plan, int precision, int kind, const gfft_iodim *cols, const gfft_iodim *rows,
                                const gfft_iodim *planes, int in_blocks, int64_t in_block_stride, int out_blocks,
                                int64_t out_block_stride);
/* Layouts of INTERNAL exchange buffers (between two stages of a distributed transform; never of a
 * caller's array, which keeps the reference's C order, pencil.py:347-354).  All three act on one-pass
 * plans (gfft_plan_create_guru, or gfft_plan_create on one axis) and return GFFT_ERR_UNSUPPORTED,
 * leaving the plan as it was, when the plan's kernel cannot address the layout.
 *
 * gfft_plan_set_tiles: `side` (0 input, 1 output) is tile-major in tiles of `tile` elements (a power
 *   of two; 0 = off) that start `tile_stride` elements apart.  For a plan along a contiguous axis the
 *   TRANSFORMED axis is tiled: entry e of a line at (e / tile) * tile_stride + e % tile from the line's
 *   base (block starts -- gfft_plan_create_guru's in_blocks / out_blocks -- stay where they were).  For a
 *   strided plan the adjacent COLUMNS (last batch dim) are tiled: column i at (i / tile) * tile_stride +
 *   i % tile.  One describes the writer, the other the reader of the same buffer: the strided stage's
 *   tile of adjacent columns is then one contiguous run per workgroup (tools/stage_layout_probe.py).
 * gfft_plan_set_flat: a strided plan walks tiles over the FLATTENED (second-last, last) batch dims, so
 *   its accesses are line aligned on a side whose rows lie back to back whatever their width (513-wide
 *   half spectra).  body_width > 0: on the INPUT side a row is stored as `body_width` columns at the
 *   planned strides plus its remaining columns at tail_offset + row * tail_row_stride (elements from
 *   the outermost batch index's base) -- the layout a neighbouring stage writes with two plans.
 * gfft_plan_set_split_slabs: gfft_plan_set_split for the half-spectrum side of packed-real rows, the
 *   rows taken as slabs of `rows_per_slab`: block b of slab s is stored as its rows cut to the body
 *   columns (w_b rounded down to whole `tile` entries; `tile` = 256 bytes of complex values), [row][body],
 *   followed by the leftover columns [row][w_b mod tile]; a block's slabs lie back to back, the blocks
 *   one after the other (same message sizes as gfft_plan_set_split).  Rows of the 513-wide block of a
 *   2048-point real axis are then 512 entries = whole 128-byte lines, for this plan's stores and for
 *   the strided plan that reads them.  (Tile-major bodies -- what complex row plans write for free --
 *   cost the packed-real kernels 18-25 % in per-entry address arithmetic, profiles/r03_stage_probe*.txt.) */
int gfft_plan_set_tiles(gfft_plan plan, int side, int tile, int64_t tile_stride);
int gfft_plan_set_flat(gfft_plan plan, int64_t body_width, int64_t tail_offset, int64_t tail_row_stride);
int gfft_plan_set_split_slabs(gfft_plan plan, int side, int nblocks, int64_t rows_per_slab, int tile);
int gfft_plan_describe(gfft_plan plan, char *buf, size_t len);
/* flops (5 n log2 n per line, half for real) and algorithmic bytes (one read + one write of
 * the array per 1-D pass) of one execute, and the number of kernel launches it issues */
int gfft_plan_cost(gfft_plan plan, double *flops, double *bytes, int *launches);

/* ---- global-redistribution helpers (what Alltoallw's datatype engine does) ------------
 * An array of shape `shape[ndims]` is cut along `axis` into `nparts` blocks by the reference's
 * block rule (pencil.py:5-9).  pack: block i is copied, in row-major order of the sub-block, to
 * d_packed + offset_i (offset_i = itemsize * prod(other dims) * start_i), i.e. the send buffer of
 * an all-to-all.  unpack is the inverse (receive buffer -> array).  itemsize in bytes (4,8,16).
 * Base alignment of these and of gfft_truncate / gfft_pad / gfft_scale below: every array as ONE of its items
 * (itemsize bytes here; 2 * precision for the complex arrays of gfft_truncate / gfft_pad; precision for
 * gfft_scale), GFFT_ERR_INVALID otherwise -- and no more: a view into a larger allocation is a valid argument.
 * gfft_pack / gfft_unpack move 16 bytes per lane where both bases are 16-byte aligned and a row of the inner
 * dims is a multiple of 16 bytes, one item per lane otherwise, with the same result.  The two arrays must not
 * overlap.  Nothing outside the `prod(shape)` items of either array is read or written. */
int gfft_pack(const void *d_array, void *d_packed, int ndims, const int64_t *shape, int axis,
              int nparts, int itemsize, void *stream);
int gfft_unpack(const void *d_packed, void *d_array, int ndims, const int64_t *shape, int axis,
                int nparts, int itemsize, void *stream);

/* ---- 3/2-rule truncation / padding along one axis (libfft.py:263-311) ------------------
 * shapes differ only along `axis` (n_padded vs n_trunc entries).  is_real: the axis is the
 * Hermitian half-axis of an r2c transform.  Element type complex<precision>.  `scale` is applied
 * to every written element (fuses `*= M`).  */
int gfft_truncate(const void *d_padded, void *d_trunc, int ndims, const int64_t *shape_padded,
                  int axis, int64_t n_trunc, int is_real, int precision, double scale, void *stream);
int gfft_pad(const void *d_trunc, void *d_padded, int ndims, const int64_t *shape_padded,
             int axis, int64_t n_trunc, int is_real, int precision, void *stream);

/* d_data[i] *= scale for `count` real scalars of the given precision */
int gfft_scale(void *d_data, int64_t count, int precision, double scale, void *stream);

/* ---- the pseudo-spectral caller either side of the path ----
 * One-pass device versions of the pointwise steps examples/spectral_dns_solver.py:65-91 writes as
 * numpy expressions.  Vector fields are [3][n0][n1][n2] (the layout of newDistArray(fft, rank=1));
 * d_k0/1/2 are the local wavenumbers along each axis (n0, n1, n2 real scalars: the sparse form of
 * get_local_wavenumbermesh, :52-63), not array-sized meshes.
 *   gfft_ps_curl     out = 1j * (K x u_hat)                                   compute_curl, :76-80
 *   gfft_ps_cross    out = a x b, real fields, count = n0*n1*n2 per component   cross, :69-74
 *   gfft_ps_project  P = sum(du*K/|K|^2); du -= P*K; du -= nu*|K|^2*u_hat      compute_rhs, :88-90
 *   gfft_ps_rk_stage u = u0 + cb*du (skipped when d_u is NULL); u1 += ca*du; `count` real scalars   :112-116
 *                    The contract of these four.  Layouts: d_u_hat, d_du_hat and d_out of gfft_ps_curl are complex
 *                    [3][n0][n1][n2], contiguous, of `precision` (GFFT_F32 / GFFT_F64), as are the vectors d_k0/1/2 (real); d_a,
 *                    d_b and d_out of gfft_ps_cross are real [3][count]; the four operands of gfft_ps_rk_stage are `count`
 *                    contiguous real scalars each (a complex field counts twice its values).  Every value is formed in the
 *                    field's precision: nu, cb and ca are converted to it once.  K is applied as given: no wavenumber is
 *                    treated specially but |K|^2 = 0, which the projection divides by 1 instead (du comes back in value).
 *                    Real and imaginary parts never mix except through the factor i of the curl, so a NaN in one part of one
 *                    operand of a mode reaches the parts of that mode it feeds and no other mode.
 *                    Read only: d_u_hat, d_k0/1/2, d_a, d_b, d_u0, d_du.  Written: d_out (every element; not read), d_du_hat
 *                    (in place, mode by mode), d_u (every element; not read) and d_u1 (in place).  d_out overlaps no input;
 *                    d_du_hat does not overlap d_u_hat; d_u and d_u1 overlap each other and the other operands nowhere (d_u0
 *                    is read only when d_u is given).  An empty block (n0 n1 n2 = 0, count = 0) launches nothing and is
 *                    GFFT_OK.  GFFT_ERR_INVALID before a device is touched for: a null pointer -- any but d_u, and d_u0 when
 *                    d_u is NULL --, a negative extent or count, a precision other than GFFT_F32 / GFFT_F64.  All four
 *                    only enqueue on `stream`: no synchronisation, no allocation.
 *   gfft_ps_spectrum shell spectrum of u_hat[ncomp][n0][n1][n2] in ONE read, every mode in double whatever the precision:
 *                      b = floor(sqrt(k0^2 + k1^2 + k2^2) / dk + 0.5)      (modes with b >= nbins are dropped)
 *                      e = 0.5 * w2[i2] * sum_c |u_hat_c|^2                (d_w2 NULL: weight 1)
 *                      out[0][b] += e;  out[1][b] += |k|^2 e               d_out = double[2][nbins], OVERWRITTEN
 *                    d_w2 carries the Hermitian double count of an r2c layout (1 at k2 = 0 and at the Nyquist column, 2
 *                    elsewhere); d_k* / d_w2 are real vectors of the transform's precision.  For forward-normalised u_hat
 *                    sum(out[0]) = <u.u>/2 and sum(out[1]) = <|grad u|^2>/2 (the enstrophy of a solenoidal field).
 *                    Partial sums of the workgroups go through the stream's scratch (allocated by the first call; run it
 *                    once before capturing it) and are added in a fixed order, no global floating-point atomics.
 *                    Inside a workgroup the waves add to a shared histogram in arrival order, so a bin repeats from one
 *                    call to the next to rounding (a few units in the last place), not bit for bit.
 *                    nbins <= 4096 and n1, n2 <= 2^30, else GFFT_ERR_UNSUPPORTED; bad arguments (null pointers other
 *                    than d_w2, ncomp < 1, nbins < 1, dk <= 0, precision) are GFFT_ERR_INVALID before a device is
 *                    touched; an empty block (n0 n1 n2 = 0) writes zeros.
 *   gfft_ps_cospectrum shell co-spectrum of a_hat and b_hat, both [ncomp][n0][n1][n2], in ONE read of each, in double as above:
 *                      b = floor(sqrt(k0^2 + k1^2 + k2^2) / dk + 0.5)      (modes with b >= nbins are dropped)
 *                      GFFT_PS_DOT       c = sum_comp Re(conj(a_c) b_c) = sum_comp (Re a_c Re b_c + Im a_c Im b_c)
 *                      GFFT_PS_HELICITY  c = Re(conj(a) . (i K x a)) = 2 K . (Re a x Im a); ncomp = 3, d_b_hat is not read
 *                                        (may be NULL) and no curl is stored
 *                      e = scale * w2[i2] * c                              (d_w2 NULL: weight 1)
 *                      out[0][b] += e;  out[1][b] += |k|^2 e               d_out = double[2][nbins], OVERWRITTEN
 *                    The bins are signed.  d_a_hat == d_b_hat is allowed: GFFT_PS_DOT of a field with itself at scale = 0.5
 *                    is gfft_ps_spectrum to rounding.  With u_hat and the projected nonlinear term N_hat (scale = 1) row 0
 *                    is the transfer spectrum T(k) of dE(k)/dt = T(k) - 2 nu k^2 E(k); GFFT_PS_HELICITY of u_hat gives H(k),
 *                    sum(out[0]) = <u . curl u>.  d_w2, d_k*, scratch, summation order, repeatability and capture: as for
 *                    gfft_ps_spectrum.
 *                    nbins <= 4096 and n1, n2 <= 2^30, else GFFT_ERR_UNSUPPORTED; bad arguments (null pointers other
 *                    than d_w2 and, for GFFT_PS_HELICITY, d_b_hat; an unknown op; ncomp < 1, or != 3 for GFFT_PS_HELICITY;
 *                    nbins < 1; dk <= 0; a non-finite scale; negative extents; precision) are GFFT_ERR_INVALID before a
 *                    device is touched; an empty block (n0 n1 n2 = 0) writes zeros.
 *   gfft_ps_stats    physical-space statistics of a REAL field u[ncomp][count] (components `count` scalars apart) in ONE
 *                    read, every value converted to double before any arithmetic; d_out = double[GFFT_PS_STATS_HEAD +
 *                    GFFT_PS_STATS_PER_COMP * ncomp] on the device, OVERWRITTEN:
 *                      out[0]          = max over points of sum_c |u_c| * inv_dx[c]   (advective CFL rate: dt <= C / out[0])
 *                      out[1]          = max over points of sum_c u_c^2
 *                      out[2 + 6c + 0] = max u_c        out[2 + 6c + 1] = min u_c
 *                      out[2 + 6c + 2] = sum u_c        out[2 + 6c + 3] = sum u_c^2
 *                      out[2 + 6c + 4] = sum u_c^3 as (u u) u              out[2 + 6c + 5] = sum u_c^4 as (u u)(u u)
 *                    inv_dx: `ncomp` HOST doubles (N_i / L_i of the grid; entries may be 0), passed by value in the launch.
 *                    NaN: the sums propagate it -- a NaN anywhere in component c makes its four sums NaN, which is the
 *                    blow-up signal to test for; the extrema follow fmax / fmin and ignore it, so out[0], out[1] and the
 *                    max / min skip a point whose value is NaN.
 *                    The result repeats BIT FOR BIT from one call to the next for the same array, count and alignment:
 *                    lanes add their own points in index order, lanes of a wave, waves of a workgroup and the workgroups'
 *                    partial results (in the stream's scratch, allocated by the first call: run it once before capturing
 *                    it) combine in a fixed tree; no floating-point atomics.
 *                    An empty block (count = 0) writes the identities: out[0] = out[1] = 0, max = -inf, min = +inf, sums 0.
 *                    ncomp > 4 is GFFT_ERR_UNSUPPORTED; bad arguments (a null pointer, ncomp < 1, count < 0, an inv_dx
 *                    entry that is negative or not finite, precision) are GFFT_ERR_INVALID before a device is touched.
 *   gfft_ps_timestep one tiny kernel on the output of gfft_ps_stats, r = d_stats[0]:
 *                      want = (r > 0 and finite) ? cfl / r : dt_max;   d_dt[0] = min(max(want, dt_min), dt_max);
 *                      d_dt[1] += d_dt[0]                                   (the running simulation time)
 *                    d_dt = double[2] on the device.  GFFT_ERR_INVALID unless cfl > 0, 0 <= dt_min <= dt_max, all finite.
 *   gfft_ps_rk_stage_dt  gfft_ps_rk_stage with the coefficients cb * d_dt[0] and ca * d_dt[0]: the products are formed in
 *                    double on the device and rounded to the field's precision as gfft_ps_rk_stage rounds its arguments,
 *                    so the result is bit for bit that of gfft_ps_rk_stage(..., cb * dt, ca * dt, ...).  A captured launch
 *                    reads d_dt[0] at every replay: with gfft_ps_stats and gfft_ps_timestep in front of it a whole
 *                    CFL-controlled step replays from one graph.
 *                    All three only enqueue on `stream`: no synchronisation, no allocation after a stream's first call.
 *   gfft_ps_force_gain   one tiny kernel on the output of gfft_ps_spectrum (d_spec = double[2][nbins]; row 0 is read): the gain
 *                    of a linear band forcing that injects energy at the rate eps,
 *                      E_f = d_spec[blo] + d_spec[blo + 1] + ... + d_spec[bhi]      (one thread, in that order)
 *                      d_gain[0] = min(eps / (2 E_f), gain_max)  where E_f > 0 and finite, else 0;   d_gain[1] = E_f
 *                    d_gain = double[2] on the device.  GFFT_ERR_INVALID (before a device is touched) for a null pointer,
 *                    nbins < 1, blo < 0, bhi < blo, bhi >= nbins, eps negative or not finite, gain_max NaN or <= 0
 *                    (+inf: no clamp).  Only enqueues.
 *   gfft_ps_project_forced   gfft_ps_project and, AFTER the projection and the viscous term, for every mode whose shell
 *                    b = floor(sqrt(k0^2 + k1^2 + k2^2) / dk + 0.5) (the expression of gfft_ps_spectrum, in double) satisfies
 *                    blo <= b <= bhi:  du_hat_c += g * u_hat_c, g = d_gain[0] (read on the device at run time) or, d_gain
 *                    NULL, `gain`; either is converted to the field's precision once, so the same double gives the same
 *                    bits both ways.  With g from gfft_ps_force_gain on the spectrum of u_hat the injected power
 *                    sum w Re(conj(u_hat) . g u_hat) = 2 g E_f is eps.  The term is not projected: it is solenoidal where
 *                    u_hat is.  One pass over the same arrays as gfft_ps_project; outside the band the result is bit for
 *                    bit that of gfft_ps_project.  A captured launch follows whatever d_gain[0] holds at each replay.
 *                    GFFT_ERR_INVALID (before a device is touched) as gfft_ps_project and for dk <= 0, blo < 0, bhi < blo,
 *                    a non-finite `gain` with d_gain NULL; n1, n2 > 2^30 is GFFT_ERR_UNSUPPORTED.  Only enqueues.
 *   gfft_ps_project_dealiased   gfft_ps_project (forced == 0) or gfft_ps_project_forced (forced != 0; dk, blo, bhi, gain, d_gain
 *                    as there, ignored otherwise) with the dealiasing truncation fused in.  Mode (i0, i1, i2) is KEPT iff
 *                      d_m0[i0] && d_m1[i1] && d_m2[i2]    three per-axis byte vectors on the device (n0, n1, n2 entries, non-zero =
 *                                                          keep): a box mask in the sparse form of d_k*; NULL keeps the whole axis
 *                      and  k0^2 + k1^2 + k2^2 <= kcut^2   as (k0 k0 + k1 k1) + k2 k2 in double from wavenumbers converted to
 *                                                          double first (the |k|^2 of gfft_ps_spectrum), kcut * kcut formed once
 *                                                          on the host; the edge is INCLUSIVE; kcut = +inf: no spherical cut,
 *                                                          at no cost (a NaN wavenumber fails a finite cut)
 *                    and TRUNCATED otherwise.  A kept mode is bit for bit the result of gfft_ps_project / gfft_ps_project_forced.
 *                    A truncated mode is +0.0 in both parts of its three components whatever du_hat and u_hat hold there (NaN
 *                    included): the predicate is evaluated before anything is loaded, and a truncated mode loads nothing.  The
 *                    2/3 rule is the box mask keeping integer wavenumber n_i iff 3 |n_i| < N_i (strictly: |n_i| <= 21 of N = 64),
 *                    after which the product of two truncated fields on the N-grid has no aliasing error in the kept modes.
 *                    One pass, no more bytes than gfft_ps_project.  GFFT_ERR_INVALID (before a device is touched) as
 *                    gfft_ps_project, for a NaN or negative kcut and, when forced != 0, as gfft_ps_project_forced; n1, n2 > 2^30
 *                    is GFFT_ERR_UNSUPPORTED.  Only enqueues.
 *   gfft_ps_dealias  the same truncation alone, in place on d_field = [ncomp][n0][n1][n2] complex: +0.0 to both parts of every
 *                    component of every truncated mode.  Kept modes are neither read nor written -- no element of the field is
 *                    read at all, so a NaN, a -0.0 or a denormal in a kept mode stays as it is.  d_k* are read only for a
 *                    spherical cut and may be NULL when kcut = +inf.  GFFT_ERR_INVALID (before a device is touched) for a null
 *                    field, ncomp < 1, negative extents, a NaN or negative kcut, a null d_k* unless kcut = +inf, precision;
 *                    n1, n2 > 2^30 is GFFT_ERR_UNSUPPORTED.  Only enqueues.
 *   Passive scalars, d theta / dt + u . grad theta = kappa lap theta - G . u (G: an imposed mean gradient, optional), in FLUX
 *   form: u . grad theta = div(u theta) for solenoidal u -- one backward and three forward transforms per scalar, as the gradient
 *   form, and no stored gradient.  Both kernels take nscalar = 1 ... 4 scalars at once and read the velocity ONCE for all of them.
 *   gfft_ps_scalar_flux  flux[s][c][e] = u[c][e] * theta[s][e] on real fields: d_u = [3][count], d_theta = [nscalar][count],
 *                    d_flux = [nscalar][3][count].  One multiply: bit for bit the correctly rounded product in the field's
 *                    precision.  3 + nscalar loads and 3 nscalar stores per point; a lane moves 16 bytes per load and store
 *                    where they divide `count` and all three bases are 16-byte aligned, one element otherwise.  d_flux must
 *                    not overlap an input.  GFFT_ERR_INVALID (before a device is touched) for a null pointer, nscalar < 1,
 *                    count < 0, precision; nscalar > 4 is GFFT_ERR_UNSUPPORTED.  Only enqueues.
 *   gfft_ps_scalar_rhs   per mode and scalar s, in the field's precision, with kk = k0 k0 + k1 k1 + k2 k2 as gfft_ps_project forms it:
 *                      a = k0 F[s][0] + k1 F[s][1] + k2 F[s][2]                              F = d_flux_hat = [nscalar][3][n0][n1][n2]
 *                      d[s] = -i a - (kappa[s] kk) theta[s] - (G[s][0] u0 + G[s][1] u1 + G[s][2] u2)      -i a = (Im a, -Re a)
 *                    d = d_dtheta_hat and theta = d_theta_hat = [nscalar][n0][n1][n2], u = d_u_hat = [3][n0][n1][n2].  kappa
 *                    (nscalar HOST doubles) and grad (nscalar x 3 HOST doubles, G[s][c] = grad[3 s + c]) travel by value in
 *                    the launch.  grad NULL: no mean-gradient term, and d_u_hat (which may be NULL) is not read at all; with
 *                    grad, d_u_hat is loaded once per mode for all scalars.  One pass: 4 nscalar (+ 3) complex loads and
 *                    nscalar stores per mode.  d_m0/1/2 and kcut select the kept modes exactly as for
 *                    gfft_ps_project_dealiased (all three NULL and kcut = +inf: every mode, at no cost): the predicate is
 *                    evaluated before anything of the mode is loaded, a truncated mode loads nothing and stores +0.0 to both
 *                    parts of its nscalar outputs whatever the inputs hold there (NaN included), a kept mode is bit for bit
 *                    the result of the call without a mask.  d_dtheta_hat must not overlap an input.  GFFT_ERR_INVALID
 *                    (before a device is touched) as gfft_ps_project_dealiased and for nscalar < 1, a null kappa, a kappa that
 *                    is negative or not finite, grad without d_u_hat, a grad that is not finite; nscalar > 4 and n1, n2 > 2^30
 *                    are GFFT_ERR_UNSUPPORTED.  Only enqueues and allocates nothing, so it can be captured.
 *   gfft_ps_rk_stage_if  one Runge-Kutta stage with an integrating factor: the linear term -nu |K|^2 u_hat (viscosity, diffusion)
 *                    is integrated exactly, so nu k_max^2 h does not limit the step (explicit RK4 needs it <= 2.785); call
 *                    gfft_ps_project with nu = 0 and gfft_ps_scalar_rhs with kappa = 0 for the right-hand side.  On complex
 *                    fields [ncomp][n0][n1][n2], ncomp = 1 ... 4, per mode and component c, in the field's precision, with
 *                    kk = k0 k0 + k1 k1 + k2 k2 as gfft_ps_project forms it, hh = (real)(h / 2), cbh = (real)(cb h), cah = (real)(ca h):
 *                      E = exp(-(((real)nu[c] kk) hh));   E^2 = E * E;   E^0 = 1 (the constant, whatever E is)
 *                      u  = E^q0 u0 + (cbh E^qd) du       (skipped when d_u is NULL; q0, qd are still checked)
 *                      u1 = E^q1 u1 + (cah E^qa) du
 *                    each update one fused multiply-add on a rounded product, fma(cbh E^qd, du, E^q0 u0), per real part.  The
 *                    powers are 0, 1 or 2.  Classical IFRK4 with u0 = u1 = u_n before the first stage is, as (cb, ca, q0, qd,
 *                    q1, qa):  (1/2, 1/6, 1, 1, 2, 2), (1/2, 1/3, 1, 0, 0, 1), (1, 1/3, 2, 1, 0, 1) and, d_u NULL,
 *                    (-, 1/6, -, -, 0, 0); u1 is then u_{n+1}.  nu (ncomp HOST doubles) travels by value in the launch; all
 *                    entries equal (a velocity): one exp per mode; otherwise one per component (scalars of several Schmidt
 *                    numbers in one call); a call whose powers are all 0 evaluates none.  h = d_dt[0], read on the device
 *                    when the kernel runs (a captured launch follows gfft_ps_timestep), or, d_dt NULL, `h`: the same double
 *                    gives the same bits both ways.  With every nu[c] = 0 the result is bit for bit that of
 *                    gfft_ps_rk_stage(..., cb * h, ca * h, ...).  A zero mode stays zero; a factor that underflows to 0 is the
 *                    correct result.  d_u0 and d_du are only read; d_u and d_u1 overlap nothing else.  One pass: the three loads
 *                    and two stores per value of gfft_ps_rk_stage and three cached wavenumber lookups per mode.
 *                    GFFT_ERR_INVALID (before a device is touched) for a null d_u1, d_du, nu or d_k*, d_u without d_u0,
 *                    ncomp < 1, negative extents, a nu that is negative or not finite, a power outside 0 ... 2, a non-finite h
 *                    with d_dt NULL, precision; ncomp > 4 and n1, n2 > 2^30 are GFFT_ERR_UNSUPPORTED.  Only enqueues and
 *                    allocates nothing, so it can be captured.
 *   The velocity-gradient tensor A_ij = d u_i / d x_j and the small-scale statistics that are functions of it: the spectral
 *   gradient of up to four fields in one pass, nine backward transforms, and ONE read of A that reduces it to 20 numbers.
 *   gfft_ps_gradient out[c][j] = i k_j f[c] on complex fields: d_f_hat = [ncomp][n0][n1][n2], d_out = [ncomp][3][n0][n1][n2] (for
 *                    ncomp = 3 the layout of newDistArray(fft, rank=2)), ncomp = 1 ... 4.  Formed as {-(k_j * Im f), k_j * Re f} in
 *                    the field's precision: each part is ONE multiply, the correctly rounded product, so the result is defined
 *                    bit for bit, the sign of a zero included; a NaN stays in its own mode and part.  K is applied as given, the
 *                    convention of gfft_ps_curl: no special case for the Nyquist columns, whose derivative is not real -- the
 *                    2/3 mask (gfft_ps_dealias, gfft_ps_project_dealiased) removes them, and a field that has been through it
 *                    has none.  One pass: ncomp complex loads, 3 ncomp stores and three cached wavenumber lookups per mode.
 *                    d_out overlaps nothing.  GFFT_ERR_INVALID (before a device is touched) for a null pointer, ncomp < 1,
 *                    negative extents, precision; ncomp > 4 and n1, n2 > 2^30 are GFFT_ERR_UNSUPPORTED.  An empty block launches
 *                    nothing.  Only enqueues and allocates nothing, so it can be captured.
 *   gfft_ps_gradient_stats   statistics of a REAL tensor field d_A = [3][3][count], A[i][j] = d u_i / d x_j (components `count`
 *                    scalars apart: the nine backward transforms of gfft_ps_gradient's output for a velocity), in ONE read, every
 *                    value converted to double before any arithmetic.  Per point, with a_ij = A[i][j] and the association
 *                    written out (the compiler may contract a product and the add that follows it into a fused multiply-add):
 *                      div = (a00 + a11) + a22                       s01 = 0.5 (a01 + a10), s02 = 0.5 (a02 + a20), s12 = 0.5 (a12 + a21)
 *                      w0 = a21 - a12, w1 = a02 - a20, w2 = a10 - a01                      (the vorticity)
 *                      d2 = (a00 a00 + a11 a11) + a22 a22            p01 = s01 s01, p02 = s02 s02, p12 = s12 s12
 *                      ss = d2 + 2 ((p01 + p02) + p12)                                     S_ij S_ij, S = (A + A^T) / 2
 *                      ww = (w0 w0 + w1 w1) + w2 w2
 *                      Q  = 0.5 (div div - (d2 + 2 ((a01 a10 + a02 a20) + a12 a21)))       ((tr A)^2 - tr(A^2)) / 2
 *                      R  = -((a00 (a11 a22 - a12 a21) - a01 (a10 a22 - a12 a20)) + a02 (a10 a21 - a11 a20))      -det A
 *                      d3 = (a00 (a00 a00) + a11 (a11 a11)) + a22 (a22 a22)
 *                      sss = (d3 + 3 ((a00 (p01 + p02) + a11 (p01 + p12)) + a22 (p02 + p12))) + 6 ((s01 s02) s12)      S_ij S_jk S_ki
 *                      wsw = ((a00 (w0 w0) + a11 (w1 w1)) + a22 (w2 w2)) + 2 ((s01 (w0 w1) + s02 (w0 w2)) + s12 (w1 w2))      w_i S_ij w_j
 *                    Q and R are the general invariants: no trace-free assumption is made.  d_out = double[GFFT_PS_GRAD_NVAL] on
 *                    the device, OVERWRITTEN:
 *                      [0] max ss       [1] max ww        [2] max |div|    [3] sum div div   [4] sum ss
 *                      [5] sum ww       [6] sum ss ss     [7] sum ww ww    [8] sum ss ww     [9] sum Q
 *                      [10] sum R       [11] sum Q Q      [12] sum R R     [13] sum sss      [14] sum wsw
 *                      [15] sum d2                        sum_i A_ii^2     (longitudinal derivatives)
 *                      [16] sum d3                        sum_i A_ii^3
 *                      [17] sum ((a00 a00)(a00 a00) + (a11 a11)(a11 a11)) + (a22 a22)(a22 a22)                    sum_i A_ii^4
 *                      [18] sum ((a01 a01 + a10 a10) + (a02 a02 + a20 a20)) + (a12 a12 + a21 a21)                 sum_{i != j} A_ij^2
 *                      [19] the same with every a a replaced by (a a)(a a)                                        sum_{i != j} A_ij^4
 *                    For a solenoidal, alias-free periodic field (Betchov): [4] = [5] / 2, [9] = [10] = 0, [14] = -4/3 [13], and
 *                    pointwise R = -(sss / 3 + wsw / 4) -- how far a run is from these tells whether it is resolved.
 *                    NaN: the sums propagate it -- a NaN in one a_ij makes every sum that reads a_ij NaN ([15] ... [17] read the
 *                    diagonal only, [18] and [19] the rest) --; the maxima follow fmax and skip a point whose value is NaN.
 *                    Launch geometry, summation order, scratch and repeatability are those of gfft_ps_stats: a lane loads 16
 *                    bytes per component where they divide `count` and d_A is 16-byte aligned, one element otherwise; the result
 *                    repeats BIT FOR BIT from one call to the next for the same array, count and alignment; no floating-point
 *                    atomics; the partial results of the workgroups go through the stream's scratch (no more of it than
 *                    gfft_ps_stats asks for; allocated by the first call: run it once before capturing it).  An empty block
 *                    (count = 0) writes zeros.  GFFT_ERR_INVALID (before a device is touched) for a null pointer, count < 0,
 *                    precision.  Only enqueues.
 *   The distributions behind those moments: histograms in ONE read, as int64 counts.  Counts are integers, so a result is exact,
 *   independent of the order in which the points arrive, repeats bit for bit and adds over ranks in any order.
 *   THE BIN RULE, the same everywhere: for a value x, converted to double before any arithmetic, a range [lo, hi) and
 *   w = (double)nbins / (hi - lo), formed ONCE on the host,
 *                      t = (x - lo) * w          (a subtraction, then a multiply: nothing a compiler may contract, so one
 *                                                 defined sequence of IEEE double operations that any host can restate)
 *                      x NaN        -> the NaN slot
 *                      t < 0        -> below
 *                      t >= nbins   -> above     (+inf, hi itself and a value within rounding of hi: the upper edge is exclusive)
 *                      otherwise    -> bin (int)t
 *   gfft_ps_histogram   the histograms of the ncomp <= 4 components of a REAL field d_u = [ncomp][count] (the layout of
 *                    gfft_ps_stats) in one read, component c over its own range [lo[c], hi[c]) (HOST doubles, by value in the
 *                    launch) with `nbins` bins each.  d_out = int64[ncomp][nbins + GFFT_PS_PDF_TAIL] on the device, OVERWRITTEN:
 *                    out[c][0 .. nbins - 1] the bins, then out[c][nbins] = below, [nbins + 1] = above, [nbins + 2] = NaN; the
 *                    entries of every component add up to `count`.
 *   gfft_ps_gradient_pdf   the histogram of one, or the joint histogram of two, of the per-point quantities of
 *                    gfft_ps_gradient_stats on d_A = [3][3][count]: GFFT_PS_Q_SS, _WW, _DIV, _Q, _R, _SSS, _WSW name ss, ww, div,
 *                    Q, R, sss and wsw with the expressions and associations written out above.  Here FMA contraction is
 *                    switched OFF: every operation of those expressions is rounded on its own, so each quantity is exactly
 *                    the value the same expression gives in IEEE double arithmetic on any host, and the counts can be compared
 *                    for equality (gfft_ps_gradient_stats itself stays as it is).  Only the quantities named by qx and qy are
 *                    evaluated; A is read once.  A NaN in a_ij reaches the quantities that read a_ij only (div reads the
 *                    diagonal alone, ww everything but the diagonal).
 *                    qy == GFFT_PS_Q_NONE (then nby must be 1, ylo and yhi are ignored): d_out = int64[nbx + 3], laid out as one
 *                    component of gfft_ps_histogram.  Otherwise the joint table d_out = int64[nbx * nby + 2]: bin bx * nby + by,
 *                    then [nbx nby] = outside, counted when either coordinate is below or above its range, then [nbx nby + 1]
 *                    = NaN, counted when either quantity is NaN (this wins over outside).  The entries add up to `count`.
 *                    Both: the launch geometry of gfft_ps_stats (16 bytes per lane and component where they divide `count` and
 *                    the base is 16-byte aligned, one element otherwise); 32-bit counters in a workgroup's LDS, bumped by
 *                    integer LDS adds, go through the stream's scratch (about 32 MiB at most, a quarter of what
 *                    gfft_ps_spectrum asks for at its bin limit; allocated by a stream's first call: run it once before capturing it) and are summed to
 *                    int64; no floating-point atomics.  An empty block (count = 0) writes zeros to all of d_out.
 *                    GFFT_ERR_INVALID (before a device is touched) for a null pointer, ncomp < 1, count < 0, a bin count < 1, a
 *                    range that is not finite, has lo >= hi or whose hi - lo or w is not finite, an unknown quantity, qx ==
 *                    GFFT_PS_Q_NONE, qy == GFFT_PS_Q_NONE with nby != 1, precision.  GFFT_ERR_UNSUPPORTED for ncomp > 4, nbins
 *                    > 4096 (gfft_ps_histogram: per component), nbx > 4096 in a 1-D and nbx * nby > 16384 in a joint
 *                    gfft_ps_gradient_pdf (64 KiB of 32-bit counters: the LDS a workgroup gets without opting in to more), and
 *                    for a count so large that one workgroup's chunk would reach 2^32 points (2^41 points and beyond).
 *                    Both only enqueue: no synchronisation, no allocation after the stream's first call. */
enum { GFFT_PS_DOT = 0, GFFT_PS_HELICITY = 1 };
enum { GFFT_PS_STATS_HEAD = 2, GFFT_PS_STATS_PER_COMP = 6 };
enum { GFFT_PS_GRAD_NVAL = 20 };
enum { GFFT_PS_PDF_TAIL = 3 };   /* after the bins of a 1-D histogram: [below] [above] [NaN] */
enum { GFFT_PS_Q_NONE = -1, GFFT_PS_Q_SS = 0, GFFT_PS_Q_WW, GFFT_PS_Q_DIV, GFFT_PS_Q_Q, GFFT_PS_Q_R,
       GFFT_PS_Q_SSS, GFFT_PS_Q_WSW, GFFT_PS_Q_COUNT };
int gfft_ps_curl(const void *d_u_hat, void *d_out, const void *d_k0, const void *d_k1, const void *d_k2,
                 int64_t n0, int64_t n1, int64_t n2, int precision, void *stream);
int gfft_ps_cross(const void *d_a, const void *d_b, void *d_out, int64_t count, int precision, void *stream);
int gfft_ps_project(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                    int64_t n0, int64_t n1, int64_t n2, double nu, int precision, void *stream);
int gfft_ps_rk_stage(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int64_t count, double cb,
                     double ca, int precision, void *stream);
int gfft_ps_spectrum(const void *d_u_hat, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2,
                     const void *d_w2, int64_t n0, int64_t n1, int64_t n2, double dk, int nbins, double *d_out,
                     int precision, void *stream);
int gfft_ps_cospectrum(const void *d_a_hat, const void *d_b_hat, int ncomp, int op, double scale, const void *d_k0,
                       const void *d_k1, const void *d_k2, const void *d_w2, int64_t n0, int64_t n1, int64_t n2, double dk,
                       int nbins, double *d_out, int precision, void *stream);
int gfft_ps_stats(const void *d_u, int ncomp, int64_t count, const double *inv_dx /* host, ncomp */, double *d_out,
                  int precision, void *stream);
int gfft_ps_timestep(const double *d_stats, double cfl, double dt_min, double dt_max, double *d_dt /* [2] */, void *stream);
int gfft_ps_rk_stage_dt(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int64_t count, double cb, double ca,
                        const double *d_dt, int precision, void *stream);
int gfft_ps_force_gain(const double *d_spec, int nbins, int blo, int bhi, double eps, double gain_max,
                       double *d_gain /* [2] */, void *stream);
int gfft_ps_project_forced(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                           int64_t n0, int64_t n1, int64_t n2, double nu, double dk, int blo, int bhi,
                           double gain, const double *d_gain /* NULL: use `gain` */, int precision, void *stream);
int gfft_ps_project_dealiased(void *d_du_hat, const void *d_u_hat, const void *d_k0, const void *d_k1, const void *d_k2,
                              const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                              int64_t n0, int64_t n1, int64_t n2, double nu, double kcut,
                              int forced, double dk, int blo, int bhi, double gain, const double *d_gain,
                              int precision, void *stream);
int gfft_ps_dealias(void *d_field, int ncomp, const void *d_k0, const void *d_k1, const void *d_k2,
                    const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                    int64_t n0, int64_t n1, int64_t n2, double kcut, int precision, void *stream);
int gfft_ps_scalar_flux(const void *d_u /* [3][count] */, const void *d_theta /* [m][count] */,
                        void *d_flux /* [m][3][count] */, int nscalar, int64_t count, int precision, void *stream);
int gfft_ps_scalar_rhs(void *d_dtheta_hat /* [m] */, const void *d_flux_hat /* [m][3] */, const void *d_theta_hat /* [m] */,
                       const void *d_u_hat /* [3], or NULL */, int nscalar,
                       const double *kappa /* host, m */, const double *grad /* host, m x 3, or NULL */,
                       const void *d_k0, const void *d_k1, const void *d_k2,
                       const unsigned char *d_m0, const unsigned char *d_m1, const unsigned char *d_m2,
                       int64_t n0, int64_t n1, int64_t n2, double kcut, int precision, void *stream);
int gfft_ps_rk_stage_if(void *d_u, const void *d_u0, void *d_u1, const void *d_du, int ncomp,
                        const double *nu /* host, ncomp */, const void *d_k0, const void *d_k1, const void *d_k2,
                        int64_t n0, int64_t n1, int64_t n2, double cb, double ca, int q0, int qd, int q1, int qa,
                        double h, const double *d_dt /* NULL: use h */, int precision, void *stream);
int gfft_ps_gradient(const void *d_f_hat /* [ncomp][n0][n1][n2] complex */,
                     void *d_out /* [ncomp][3][n0][n1][n2] complex */, int ncomp,
                     const void *d_k0, const void *d_k1, const void *d_k2,
                     int64_t n0, int64_t n1, int64_t n2, int precision, void *stream);
int gfft_ps_gradient_stats(const void *d_A /* [3][3][count] real, A[i][j] = d u_i / d x_j */,
                           int64_t count, double *d_out /* [GFFT_PS_GRAD_NVAL], overwritten */,
                           int precision, void *stream);
int gfft_ps_histogram(const void *d_u /* [ncomp][count] real */, int ncomp, int64_t count,
                      const double *lo, const double *hi /* host, ncomp each */, int nbins,
                      int64_t *d_out /* [ncomp][nbins + 3], overwritten */, int precision, void *stream);
int gfft_ps_gradient_pdf(const void *d_A /* [3][3][count] real */, int64_t count,
                         int qx, double xlo, double xhi, int nbx,
                         int qy, double ylo, double yhi, int nby,
                         int64_t *d_out, int precision, void *stream);

/* ---- the fields where no grid point is: B-spline interpolation at particle positions ----------
 *   gfft_ps_scale_axes   the separable spectral multiplier: out[c][i0][i1][i2] = f_hat[c][i0][i1][i2] * g with
 *                    g = (v0[i0] * v1[i1]) * v2[i2], the vectors real, of the field's precision, over the block's axes.  g is
 *                    formed in the field's precision; the real and the imaginary part are each ONE multiply by g.  A NULL
 *                    vector means that axis contributes no factor -- no multiply by 1 is issued for it (v0 NULL: g = v1 * v2;
 *                    all NULL: a copy).  Every result is a defined sequence of single multiplies with nothing to contract,
 *                    so it equals a host restatement in the same precision bit for bit, NaN, inf and the sign of a zero
 *                    included.  d_out == d_f_hat (in place) is allowed; any other overlap is not.  1 <= ncomp <= 4.
 *                    The prefilter of cubic B-spline interpolation is one such g (per axis 1 / ((2 + cos(2 pi n / N)) / 3),
 *                    n the integer wavenumber); any separable filter (Gaussian, box) is three vectors through the same call.
 *                    GFFT_ERR_INVALID (before a device is touched) for a null field, ncomp < 1, a negative size, precision;
 *                    GFFT_ERR_UNSUPPORTED for ncomp > 4 and an axis longer than 2^30.  Only enqueues.
 *   gfft_ps_interp   d_out[p][c] = the order-2 (trilinear) or order-4 (cubic B-spline) interpolant of the coefficient field
 *                    c at position x[p], restricted to the stencil points THIS block owns.  d_c = [ncomp][n[0]][n[1]][n[2]]
 *                    real, the block start[a] .. start[a] + n[a] of a periodic grid of N[a] cells per axis; inv_dx[a] = N[a] /
 *                    L[a] (host); d_x = double [np][3] whatever the field's precision; d_out = double [np][ncomp], OVERWRITTEN.
 *                    THE DEFINITION, per particle p and axis a, in double:
 *                      s = x[p][a] * inv_dx[a]                  (one multiply)
 *                      !(fabs(s) < 2^51) on ANY axis            -> every entry of out[p][:] is NaN and nothing is loaded
 *                                                                  (NaN, +-inf, and anything too large to have a fraction)
 *                      i = floor(s),  t = s - i                 (one rounded subtraction; t may come out as exactly 1.0 for a
 *                                                                  tiny negative s: the weights are continuous there)
 *                      order 2:  base b = i,      weights  1 - t,  t
 *                      order 4:  base b = i - 1,  with r = 1 - t the weights
 *                                r^3 / 6,  (3 t^3 - 6 t^2 + 4) / 6,  (3 r^3 - 6 r^2 + 4) / 6,  t^3 / 6
 *                      for stencil offset j = 0 .. order - 1:   g = (b + j) mod N[a] as a non-negative int64, l = g - start[a];
 *                                                                the point contributes iff 0 <= l < n[a] on all three axes
 *                      out[p][c] = sum over the contributing points of ((w0 * w1) * w2) * (double)c[c][l0][l1][l2]
 *                    taken in ONE fixed order (a row of the stencil along the last axis in a lane, the rows by a fixed
 *                    butterfly), so the result repeats bit for bit from call to call; a particle with no contributing
 *                    point gets +0.0.  How the weight polynomials are evaluated and whether a product is contracted into
 *                    the sum is not part of the definition: a result lies within (order^3 + 64) 2^-53 sum |w0 w1 w2 c| of the
 *                    exact sum.  Summed over the blocks of a grid the results are the full interpolant; with start = 0,
 *                    n = N it is the whole periodic interpolant.  Positions are NOT required to lie in the box: they
 *                    wrap.  N[a] < order is legal: the stencil wraps onto itself, which periodicity makes correct.  For order
 *                    4, c must hold B-spline coefficients: the backward transform of gfft_ps_scale_axes with the prefilter
 *                    above; fed samples instead it smooths.  Every index that reaches a load has gone through the integer
 *                    wrap and the block test -- or is the constant 0, element 0 of a component, read in place of a point
 *                    outside the block and dropped --, and the 2^51 guard comes before the conversion to an integer: no
 *                    position, finite or not, addresses outside the block.  A NaN in c reaches exactly the particles whose stencil
 *                    holds it (a point of weight 0 included).  np = 0 launches nothing.  order^2 lanes serve a particle;
 *                    no atomics, no scratch.  GFFT_ERR_INVALID (before a device is touched) for a null pointer, ncomp < 1,
 *                    np < 0, an order other than 2 or 4, n or N < 1, start < 0, start + n > N, an inv_dx that is not
 *                    finite and > 0, precision; GFFT_ERR_UNSUPPORTED for ncomp > 4 (and a grid axis beyond 2^40).  Only enqueues. */
int gfft_ps_scale_axes(void *d_out, const void *d_f_hat /* [ncomp][n0][n1][n2] complex */, int ncomp,
                       const void *d_v0, const void *d_v1, const void *d_v2 /* real [n0], [n1], [n2]; NULL: no factor */,
                       int64_t n0, int64_t n1, int64_t n2, int precision, void *stream);
int gfft_ps_interp(const void *d_c /* [ncomp][n[0]][n[1]][n[2]] real: this rank's block of the coefficients */,
                   int ncomp, const int64_t n[3], const int64_t start[3], const int64_t N[3],
                   const double inv_dx[3] /* host: N_i / L_i */,
                   const double *d_x /* [np][3] positions, double whatever the field's precision */,
                   int64_t np, int order /* 2 (trilinear) or 4 (cubic B-spline) */,
                   double *d_out /* [np][ncomp], overwritten */, int precision, void *stream);

/* ---- particle to grid: the transpose of gfft_ps_interp, order-independent to the last bit ----------
 *   gfft_ps_spread   d_acc[c][l0][l1][l2] += the contributions of np particles to the stencil points THIS block owns, with the
 *                    weights of gfft_ps_interp, each contribution rounded ONCE to a 64-bit integer (fixed point, 2^scale_exp
 *                    units per unit of q) and added by an integer atomic.  Integer addition is associative: d_acc does not
 *                    depend on the order in which the adds arrive, on the order of the particles or on how the grid is cut
 *                    into blocks, and a host restates it bit for bit.  d_acc = int64 [ncomp][n[0]][n[1]][n[2]], ADDED TO (the
 *                    caller zeroes it, or gfft_ps_spread_finish does); n, start, N, inv_dx, d_x as in gfft_ps_interp;
 *                    d_q = double [np][ncomp]; d_skipped = int64 [1], ADDED TO.
 *                    THE DEFINITION, per particle p, in double, EVERY operation rounded on its own (no product is contracted
 *                    into a sum or a difference):
 *                      s_a = x[p][a] * inv_dx[a]                (one multiply per axis)
 *                      u_c = q[p][c] * 2^scale_exp              (one multiply; the host forms 2^scale_exp with ldexp)
 *                      !(fabs(s_a) < 2^51) on ANY axis or !(fabs(u_c) < 2^62) for ANY component
 *                                                               -> the particle is SKIPPED: it adds nothing to any component
 *                                                                  and *d_skipped grows by one (NaN and +-inf fail both tests).
 *                                                                  This comes BEFORE the block test: every block of a grid
 *                                                                  counts the same particles
 *                      i = floor(s),  t = s - i,  r = 1 - t,  sixth = 1.0 / 6.0
 *                      order 2:  base b = i,      weights  r,  t
 *                      order 4:  base b = i - 1,  weights  ((r*r)*r)*sixth,  ((t*t)*(3.0*t - 6.0) + 4.0)*sixth,
 *                                                          ((r*r)*(3.0*r - 6.0) + 4.0)*sixth,  ((t*t)*t)*sixth
 *                      for stencil offset j = 0 .. order - 1:   g = (b + j) mod N[a] as a non-negative int64, l = g - start[a];
 *                                                                the point receives iff 0 <= l < n[a] on all three axes
 *                                                                (the wrap and the test of gfft_ps_interp)
 *                      for every receiving point and component: k = llrint(((w0 * w1) * w2) * u_c), ties to even;
 *                                                                acc[c][l0][l1][l2] += k  as a 64-bit add modulo 2^64
 *                    N[a] < order is legal: the stencil wraps onto itself and one particle adds to one address several
 *                    times.  The add is a no-return 64-bit integer atomic at agent scope; no floating-point atomic, no LDS,
 *                    no scratch.  Weights are >= 0 and sum to 1, so with 2^scale_exp * max_c sum_p |q[p][c]| <= 2^62 no
 *                    accumulator leaves int64; a point's value lies within n_l 2^-(scale_exp + 1) + 16 * 2^-53 * sum |w q| of the
 *                    exact sum (n_l contributions: half a unit each, plus the roundings of the weights and products).
 *                    Every index that reaches an add has gone through the 2^51 guard, the integer wrap and the block test.
 *                    np = 0 launches nothing.  GFFT_ERR_INVALID (before a device is touched) for a null pointer, ncomp < 1,
 *                    np < 0, an order other than 2 or 4, |scale_exp| > 1000, n or N < 1, start < 0, start + n > N, an inv_dx
 *                    that is not finite and > 0; GFFT_ERR_UNSUPPORTED for ncomp > 4 (and a grid axis beyond 2^40).  Only enqueues.
 *   gfft_ps_spread_finish   out[i] = (real)((double)acc[i] * factor) for i < count: one conversion, one multiply and, for
 *                    GFFT_F32, one narrowing; THEN, if clear != 0, acc[i] = 0 (a captured step needs no memset).  With factor =
 *                    2^-scale_exp (times a normalisation: the wrapper passes the ONE host quotient factor / 2^scale_exp) out
 *                    is the spread field.  d_out and d_acc do not overlap.  count = 0 launches nothing.  GFFT_ERR_INVALID
 *                    (before a device is touched) for a null pointer, count < 0, a factor that is not finite, precision.
 *                    Only enqueues. */
int gfft_ps_spread(int64_t *d_acc /* [ncomp][n[0]][n[1]][n[2]], ADDED to */, int ncomp,
                   const int64_t n[3], const int64_t start[3], const int64_t N[3], const double inv_dx[3],
                   const double *d_x /* [np][3] */, const double *d_q /* [np][ncomp] */, int64_t np,
                   int order /* 2 or 4 */, int scale_exp, int64_t *d_skipped /* [1], ADDED to */, void *stream);
int gfft_ps_spread_finish(void *d_out /* [count] real of `precision` */, int64_t *d_acc /* [count] */, int64_t count,
                          double factor, int clear, int precision, void *stream);

/* ---- two-point statistics in physical space: structure functions along a grid axis ----------
 *   gfft_ps_structure   the power sums of the increments of a real field over a list of separations along one periodic axis,
 *                    the field read from memory ONCE for all separations.  d_u = real [ncomp][n[0]][n[1]][n[2]], contiguous, of
 *                    `precision`: a block that spans the WHOLE periodic axis `axis` (n[axis] is that axis's period; the other
 *                    two axes may be any part of the grid); sep[0 .. nsep - 1] (host) = the separations in grid points, 0 <=
 *                    sep[k] < n[axis]; lcomp = the component that serves as the longitudinal velocity of the mixed moment,
 *                    or -1 for none; d_out = double [nsep][ncomp][GFFT_PS_SF_NVAL], OVERWRITTEN.
 *                    THE DEFINITION, for every point x of the block, separation k and component c, in double, every value
 *                    converted before any arithmetic:
 *                      a  = (double)u[c][x]
 *                      b  = (double)u[c][x'],   x' = x with index[axis] replaced by (index[axis] + sep[k]) mod n[axis]
 *                      d  = b - a
 *                      d2 = d*d    d3 = d2*d    d4 = d2*d2    d5 = d4*d    d6 = d3*d3
 *                      ad = fabs(d)    ad3 = d2*ad
 *                      mx = dl*d2      dl = the d of component lcomp at the same x and k
 *                                      (lcomp = -1: the entry is +0.0 and nothing is formed)
 *                      out[k][c][GFFT_PS_SF_D1 ... GFFT_PS_SF_MIX] = the sums over x of  d, d2, d3, d4, d5, d6, ad, ad3, mx
 *                    With u a velocity and c = lcomp = axis, D3 carries the 4/5 law; summed over c, MIX is <du_L |du|^2> of
 *                    the 4/3 law; with c a scalar it is <du_L dtheta^2> of Yaglom's law.  Whether a product is contracted
 *                    into its accumulation is not part of the definition: a sum lies within (count + 16) 2^-53 M of the
 *                    exact one, count = n[0] n[1] n[2] and M the same expression over |a|, |b| with the subtraction turned
 *                    into an addition.  THE SUMMATION ORDER is fixed, so the result repeats bit for bit for the same array,
 *                    geometry (n, axis, ncomp, nsep, precision) and 16-byte alignment of d_u.  The lines of `axis` are
 *                    cut into tiles of whole lines (axis 2: consecutive lines; axis 0 or 1: for one index of the axes in
 *                    front, a power-of-two run of consecutive columns of the axes behind), tile t served by workgroup
 *                    t mod nwg of 256 lanes; a tile's points are numbered p in its staging order (axis 2: memory order;
 *                    else [index along axis][column]); per tile and separation
 *                      1. lane l adds its points p = l, l + 256, ... in that order, from +0.0;
 *                      2. the 64 lanes of a wave combine by the butterfly lane ^ 32, 16, 8, 4, 2, 1;
 *                      3. the 4 waves add in wave order, and the result is added to the workgroup's running sum, tile
 *                         after tile in the order t = w, w + nwg, ...;
 *                    and last, per (k, c, value), lane l of one workgroup adds the workgroups' sums w = l, l + 256, ... in that
 *                    order, then 2. and 3.  No floating-point atomics.
 *                    A NaN (or an infinity, whose difference with itself is NaN) reaches exactly the sums it enters: the
 *                    sums of its own component at every separation, and the MIX entries of every component if it lies in
 *                    component lcomp.  sep = 0 gives zeros for a finite field (d = a - a).  A block with count == 0 gives
 *                    zeros and launches only the final combination.  Every index that reaches a load has gone through the
 *                    integer wrap.  The workgroups' sums live in the stream's shared scratch (at most 4 MiB): the first
 *                    call allocates, later ones only enqueue, so a captured call allocates nothing.
 *                    GFFT_ERR_INVALID (before a device is touched) for a null pointer, ncomp < 1, nsep < 1, an axis
 *                    outside 0 .. 2, a negative n, a sep outside [0, n[axis]), lcomp outside [-1, ncomp), precision;
 *                    GFFT_ERR_UNSUPPORTED for ncomp > 4, nsep > 64, n[axis] > 4096 (a workgroup stages whole lines of all
 *                    components in LDS: 128 KiB at 4096 x 4 doubles) and a block of more than 2^40 points.  Only enqueues. */
enum { GFFT_PS_SF_D1 = 0, GFFT_PS_SF_D2 = 1, GFFT_PS_SF_D3 = 2, GFFT_PS_SF_D4 = 3, GFFT_PS_SF_D5 = 4, GFFT_PS_SF_D6 = 5,
       GFFT_PS_SF_ABS1 = 6, GFFT_PS_SF_ABS3 = 7, GFFT_PS_SF_MIX = 8, GFFT_PS_SF_NVAL = 9 };
enum { GFFT_PS_SF_MAX_SEP = 64, GFFT_PS_SF_MAX_AXIS = 4096 };
int gfft_ps_structure(const void *d_u /* [ncomp][n[0]][n[1]][n[2]] real */, int ncomp, const int64_t n[3], int axis,
                      int nsep, const int32_t *sep /* host */, int lcomp /* -1: none */,
                      double *d_out /* [nsep][ncomp][GFFT_PS_SF_NVAL], overwritten */, int precision, void *stream);

/* ---- random fields: initial conditions and white-in-time forcing, keyed by the global mode index ----------
 *   gfft_ps_random_field   fills (add == 0) or adds to (add != 0) the complex field d_out[ncomp][n[0]][n[1]][n[2]] of `precision`,
 *                    the block start[a] .. start[a] + n[a] of a spectral array over the global physical grid N (a real
 *                    transform stores indices 0 .. N[2]/2 of the last axis; no flag tells the layouts apart), with
 *                    independent complex Gaussian modes of a prescribed amplitude per shell that obey u(-k) = conj u(k)
 *                    exactly.  d_k0/1/2 = the block's wavenumber vectors in the field's precision; d_amp = device
 *                    double[nbins] or NULL (every amplitude 1).  1 <= ncomp <= 4.
 *                    THE DEFINITION, per stored mode with global index g = start + i, in this order:
 *                      mirror     m = ((N0 - g0) % N0, (N1 - g1) % N1, (N2 - g2) % N2);  lin(g) = (g0 N1 + g1) N2 + g2 in
 *                                 uint64;  c = min(lin(g), lin(m));  the mode is a MIRROR MODE iff lin(m) < lin(g)
 *                      zeroed     g = 0; 2 g_a == N_a on any axis (a Nyquist index: K(m) != -K(g) there, and no self-
 *                                 conjugate mode is left once these are gone); b >= nbins, b = floor(|k| / dk + 0.5) the
 *                                 shell gfft_ps_spectrum bins by (a NaN shell too); amp[b] == 0.  A zeroed mode is stored
 *                                 as +0, or with `add` left untouched; nothing is drawn for it
 *                      uniforms   per component comp one Philox4x32-10 call, counter (c lo32, c hi32, stream_id lo32,
 *                                 (stream_id >> 32) << 2 | comp), key (seed lo32, seed hi32), words r0 .. r3:
 *                                 u1 = (((r1 << 32 | r0) >> 12) + 0.5) 2^-52, u2 the same from (r3, r2): exact doubles in (0, 1)
 *                      Gaussians  rho = sqrt(-2 log u1);  G_comp = rho (cos 2 pi u2 + i sin 2 pi u2)   (sincospi(2 u2)), in
 *                                 double whatever the precision; each part a standard normal
 *                      project    (project != 0, which needs ncomp == 3) per part, in double with the block's K converted
 *                                 first and nothing contracted:  p = ((kx G0 + ky G1) + kz G2) / |k|^2,  G_j = G_j - k_j p,
 *                                 |k|^2 = (kx kx + ky ky) + kz kz (0 -> 1).  E |u|^2 summed over the components is then 4 amp^2
 *                      store      each part times amp[b]; the imaginary part negated for a mirror mode; rounded ONCE to
 *                                 `precision`; stored, or with `add` added in `precision` to what is there
 *                    K(m) = -K(g) exactly on the surviving modes and K enters only through products of two K's, so a mirror
 *                    mode is bit for bit the conjugate of its partner: the physical field is real, the r2c field is the
 *                    stored half of the c2c field, and a mode's value does not depend on the block that holds it.  Against
 *                    the exact value of the definition a part lies within 20 x 2^-53 amp ||G||_2 (log, sqrt and sincospi at
 *                    their documented 1, 1 and 2 ulp and the roundings above; tests/random_ref.py derives it).
 *                    Pointwise, no atomics, no scratch; an empty block launches nothing.  GFFT_ERR_INVALID (before a
 *                    device is touched) for a null pointer (d_amp excepted), ncomp outside 1 .. 4, project with ncomp != 3,
 *                    nbins < 1, dk <= 0, n < 0, N < 1, start < 0, start + n > N, stream_id >= 2^62, precision;
 *                    GFFT_ERR_UNSUPPORTED for n[1] or n[2] > 2^30 and a grid of more than 2^60 points.  Only enqueues.
 *   gfft_ps_scale_shells   the isotropic counterpart of gfft_ps_scale_axes: out[c][i0][i1][i2] = f_hat[c][i0][i1][i2] *
 *                    (real)tab[b] with b the shell above, d_tab = device double[nbins]; the real and the imaginary part are
 *                    each ONE multiply, bit for bit a host restatement.  A mode with b >= nbins (a NaN shell too) is stored
 *                    as +0 whatever f_hat holds there.  d_out == d_f_hat (in place) is allowed; any other overlap is not.
 *                    Sharp and Gaussian LES filters, a rescale to an exact spectrum.  GFFT_ERR_INVALID for a null pointer,
 *                    ncomp < 1, nbins < 1, dk <= 0, a negative size, precision; GFFT_ERR_UNSUPPORTED for ncomp > 4 and an
 *                    axis longer than 2^30.  Only enqueues. */
int gfft_ps_random_field(void *d_out /* [ncomp][n[0]][n[1]][n[2]] complex */, int ncomp, const int64_t n[3],
                         const int64_t start[3], const int64_t N[3], const void *d_k0, const void *d_k1, const void *d_k2,
                         int project, double dk, const double *d_amp /* [nbins] or NULL */, int nbins, uint64_t seed,
                         uint64_t stream_id /* < 2^62 */, int add, int precision, void *stream);
int gfft_ps_scale_shells(void *d_out, const void *d_f_hat /* [ncomp][n0][n1][n2] complex */, int ncomp, const void *d_k0,
                         const void *d_k1, const void *d_k2, double dk, const double *d_tab /* [nbins] */, int nbins,
                         int64_t n0, int64_t n1, int64_t n2, int precision, void *stream);

/* ---- the wire of a global redistribution: RCCL over xGMI -------------------------------------
 * Replaces, for device buffers, what the reference gets from MPI on its Cartesian sub-communicators:
 *   gfft_comm_create / gfft_comm_split  <- MPI_Cart_create + MPI_Cart_sub   mpi4py_fft/pencil.py:64-93
 *   gfft_alltoallv / gfft_sendrecv      <- comm.Alltoallw(...)             mpi4py_fft/pencil.py:182-183,200-201
 * One process per GPU; a communicator is bound to the device current at its creation.  RCCL is
 * loaded at run time (an already loaded librccl is shared; GFFT_RCCL_LIB or gfft_rccl_load name a
 * specific one), so these entries return GFFT_ERR_UNSUPPORTED on a host without RCCL and nothing
 * else in the library depends on it.  The 128-byte unique id is produced on one rank and carried to
 * the others by whatever the host already has (MPI_Bcast, a torch.distributed store, a file).
 * All calls are collective where RCCL's are (create: all ranks; split: all ranks of the parent) and
 * every exchange is enqueued on `stream`: the host owns the stream and orders it against its compute
 * streams with events (gfft_event_record / gfft_stream_wait_event).  Error detail:
 * gfft_exchange_last_error(). */
typedef struct gfft_comm_s *gfft_comm;
typedef struct {
  void *ptr;        /* device address of the message */
  int64_t bytes;
  int peer;         /* rank in the communicator */
} gfft_msg;
#define GFFT_UNIQUE_ID_BYTES 128
int gfft_rccl_load(const char *path);                   /* NULL: default search */
int gfft_rccl_info(char *buf, size_t len);
const char *gfft_exchange_last_error(void);
int gfft_comm_get_unique_id(void *id128);
int gfft_comm_create(gfft_comm *comm, const void *id128, int nranks, int rank);
/* ranks passing the same color >= 0 form a group, ordered by key then parent rank; color < 0 joins
 * no group (*sub = NULL).  Sub-communicator of grid axis i: color = the other coordinates, key =
 * coordinate i (pencil.py:80-88). */
int gfft_comm_split(gfft_comm parent, int color, int key, gfft_comm *sub);
int gfft_comm_rank(gfft_comm comm, int *rank, int *size);
int gfft_comm_destroy(gfft_comm comm);
/* One grouped batch of point-to-point messages (ncclGroupStart .. ncclGroupEnd).  Messages
 * between two ranks match in list order; messages to oneself are device copies. */
int gfft_sendrecv(gfft_comm comm, int nsend, const gfft_msg *sends, int nrecv, const gfft_msg *recvs, void *stream);
/* MPI_Alltoallv on device buffers: send_counts[i] items at item offset send_displs[i] of d_send go
 * to rank i; recv_counts[j] items from rank j land at item offset recv_displs[j] of d_recv. */
int gfft_alltoallv(gfft_comm comm, const void *d_send, const int64_t *send_counts, const int64_t *send_displs,
                   void *d_recv, const int64_t *recv_counts, const int64_t *recv_displs, int itemsize, void *stream);
int gfft_stream_create(void **stream);                  /* non-blocking HIP stream */
int gfft_stream_destroy(void *stream);
int gfft_stream_wait_event(void *stream, void *event);
int gfft_event_create_untimed(void **event);            /* for ordering only (hipEventDisableTiming) */

/* ---- raw device helpers for non-torch hosts (the Python host uses torch for these) ---- */
int gfft_malloc(void **d_ptr, size_t bytes);
int gfft_free(void *d_ptr);
int gfft_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int gfft_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int gfft_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);
int gfft_stream_synchronize(void *stream);

/* ---- measurement helpers used by bench.py (HIP events on the launch stream) ------------ */
int gfft_event_create(void **event);
int gfft_event_record(void *event, void *stream);
int gfft_event_elapsed_ms(void *start, void *stop, float *ms);   /* synchronises on `stop` */
int gfft_event_destroy(void *event);
/* per-pass kernel timing for the roofline report: set option "profile" to 1, execute, then read
 * the accumulated milliseconds of each pass (HIP events recorded on the execute stream) */
int gfft_plan_profile(gfft_plan plan, float *ms, int max_passes, int *executes);
int gfft_plan_pass_info(gfft_plan plan, int pass, char *buf, size_t len, double *algorithmic_bytes);
/* TEST AID: tiles (units of work a workgroup takes one at a time) and workgroups of pass `pass`'s most recent launch;
 * 0 / 0 before the plan's first execute.  GFFT_ERR_INVALID: null plan or out pointer, bad pass index ("bad pass index",
 * as gfft_plan_pass_info).  GFFT_ERR_UNSUPPORTED: a persistent fused pair (its workgroups draw tickets; no cap applies). */
int gfft_plan_pass_launch(gfft_plan plan, int pass, int64_t *tiles, int *workgroups);
/* streaming-copy probe: dst[i] = src[i] over `bytes` (multiple of 16); the HBM ceiling quoted
 * beside roofline numbers */
int gfft_probe_copy(const void *d_src, void *d_dst, size_t bytes, void *stream);
/* strided-tile copy probe: the access pattern of a column pass without the arithmetic:
 * array [outer][n][inner] of 16-byte elements, tiles of `tcols` consecutive inner elements */
int gfft_probe_tile_copy(const void *d_src, void *d_dst, int64_t outer, int64_t n, int64_t inner,
                         int tcols, void *stream);
/* single-pass probe: run ONE power-of-two pass with explicit batch geometry and strides (element
 * units), bypassing the planner.  geom = {n, outer, mid, inner, in_os, in_ms, in_is, in_es, out_os,
 * out_ms, out_is, out_es}.  A measuring aid (tools/layout_probe.py), not part of the drop-in path. */
int gfft_debug_pass(const int64_t *geom, int precision, int cols, int variant, int inverse,
                    const void *d_in, void *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GFFT_H */
