"""ctypes binding of libgfft.so (include/gfft.h) and the engine object the host classes call.

There is exactly one product engine: :class:`HipEngine`, a thin veneer over the C ABI.  It has no
host fallback -- if the shared library is missing or no HIP device is visible every compute call
raises.  ``set_engine`` exists so that CPU-only unit tests of the *host logic* (pencil arithmetic,
exchange plans, gloo all-to-all) can inject a checker engine from tests/; nothing in this package
ever selects another engine on its own.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(_HERE, 'libgfft.so')

C2C_FORWARD, C2C_BACKWARD, R2C, C2R = -1, 1, -2, 2
PS_DOT, PS_HELICITY = 0, 1              # op of gfft_ps_cospectrum
PS_STATS_HEAD, PS_STATS_PER_COMP = 2, 6 # layout of gfft_ps_stats' output: double[HEAD + PER_COMP * ncomp]
PS_GRAD_NVAL = 20                       # gfft_ps_gradient_stats' output: double[PS_GRAD_NVAL], indexed by the names below
(GS_MAX_SS, GS_MAX_WW, GS_MAX_DIV, GS_DIV2, GS_SS, GS_WW, GS_SS2, GS_WW2, GS_SSWW, GS_Q, GS_R, GS_Q2, GS_R2, GS_SSS, GS_WSW,
 GS_LONG2, GS_LONG3, GS_LONG4, GS_TRANS2, GS_TRANS4) = range(PS_GRAD_NVAL)
PS_GRAD_NMAX = 3                        # entries 0 ... 2 are maxima, the rest sums
PS_PDF_TAIL = 3                         # behind the bins of a 1-D histogram: [below] [above] [NaN]
PS_Q_NONE = -1                          # gfft_ps_gradient_pdf's quantities, named as in gfft_ps_gradient_stats
PS_Q_SS, PS_Q_WW, PS_Q_DIV, PS_Q_Q, PS_Q_R, PS_Q_SSS, PS_Q_WSW, PS_Q_COUNT = range(8)
PS_PDF_MAX_BINS, PS_PDF_MAX_JOINT = 4096, 16384      # bins of a 1-D table (per component) and of a joint one
PS_SF_NVAL = 9                          # gfft_ps_structure's output: double[nsep][ncomp][PS_SF_NVAL], indexed by the names below
SF_D1, SF_D2, SF_D3, SF_D4, SF_D5, SF_D6, SF_ABS1, SF_ABS3, SF_MIX = range(PS_SF_NVAL)
PS_SF_MAX_SEP, PS_SF_MAX_AXIS = 64, 4096             # separations per call; the longest axis a workgroup stages

_lib = None


class GfftError(RuntimeError):
    pass


class IoDim(ctypes.Structure):          # gfft_iodim
    _fields_ = [('n', ctypes.c_int64), ('is_', ctypes.c_int64), ('os', ctypes.c_int64)]


class Msg(ctypes.Structure):            # gfft_msg
    _fields_ = [('ptr', ctypes.c_void_p), ('bytes', ctypes.c_int64), ('peer', ctypes.c_int)]


def _declare(lib):
    c = ctypes
    i64p = c.POINTER(c.c_int64)
    ip = c.POINTER(c.c_int)
    vp = c.c_void_p
    sigs = {
        'gfft_strerror': (c.c_char_p, [c.c_int]),
        'gfft_last_error': (c.c_char_p, []),
        'gfft_version': (c.c_int, []),
        'gfft_device_count': (c.c_int, [ip]),
        'gfft_device_name': (c.c_int, [c.c_int, c.c_char_p, c.c_size_t]),
        'gfft_set_option': (c.c_int, [c.c_char_p, c.c_int]),
        'gfft_plan_create': (c.c_int, [c.POINTER(vp), c.c_int, i64p, i64p, c.c_int, ip, c.c_int, c.c_int]),
        'gfft_plan_create_r2r': (c.c_int, [c.POINTER(vp), c.c_int, i64p, c.c_int, ip, ip, c.c_int]),
        'gfft_execute': (c.c_int, [vp, vp, vp, c.c_double, vp]),
        'gfft_plan_destroy': (c.c_int, [vp]),
        'gfft_scratch_release': (c.c_int, []),
        'gfft_plan_set_truncation': (c.c_int, [vp, c.c_int64]),
        'gfft_plan_create_padded': (c.c_int, [c.POINTER(vp), i64p, i64p, c.c_int, c.c_int]),
        'gfft_plan_set_split': (c.c_int, [vp, c.c_int, c.c_int]),
        'gfft_plan_create_guru': (c.c_int, [c.POINTER(vp), c.c_int, c.c_int, c.POINTER(IoDim), c.c_int, c.POINTER(IoDim),
                                            c.c_int, c.c_int64, c.c_int, c.c_int64]),
        'gfft_plan_create_guru_padded': (c.c_int, [c.POINTER(vp), c.c_int, c.c_int, c.POINTER(IoDim), c.c_int64, c.c_int,
                                                   c.POINTER(IoDim), c.c_int, c.c_int64, c.c_int, c.c_int64]),
        'gfft_plan_create_guru2': (c.c_int, [c.POINTER(vp), c.c_int, c.c_int, c.POINTER(IoDim), c.POINTER(IoDim), c.POINTER(IoDim),
                                             c.c_int, c.c_int, c.c_int64, c.c_int, c.c_int64]),
        'gfft_plan_create_guru2_real': (c.c_int, [c.POINTER(vp), c.c_int, c.c_int, c.POINTER(IoDim), c.POINTER(IoDim),
                                                  c.POINTER(IoDim), c.c_int, c.c_int64, c.c_int, c.c_int64]),
        'gfft_plan_set_tiles': (c.c_int, [vp, c.c_int, c.c_int, c.c_int64]),
        'gfft_plan_set_flat': (c.c_int, [vp, c.c_int64, c.c_int64, c.c_int64]),
        'gfft_plan_set_split_slabs': (c.c_int, [vp, c.c_int, c.c_int, c.c_int64, c.c_int]),
        'gfft_plan_describe': (c.c_int, [vp, c.c_char_p, c.c_size_t]),
        'gfft_plan_cost': (c.c_int, [vp, c.POINTER(c.c_double), c.POINTER(c.c_double), ip]),
        'gfft_pack': (c.c_int, [vp, vp, c.c_int, i64p, c.c_int, c.c_int, c.c_int, vp]),
        'gfft_unpack': (c.c_int, [vp, vp, c.c_int, i64p, c.c_int, c.c_int, c.c_int, vp]),
        'gfft_truncate': (c.c_int, [vp, vp, c.c_int, i64p, c.c_int, c.c_int64, c.c_int, c.c_int, c.c_double, vp]),
        'gfft_pad': (c.c_int, [vp, vp, c.c_int, i64p, c.c_int, c.c_int64, c.c_int, c.c_int, vp]),
        'gfft_scale': (c.c_int, [vp, c.c_int64, c.c_int, c.c_double, vp]),
        'gfft_ps_curl': (c.c_int, [vp, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_int, vp]),
        'gfft_ps_cross': (c.c_int, [vp, vp, vp, c.c_int64, c.c_int, vp]),
        'gfft_ps_project': (c.c_int, [vp, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double, c.c_int, vp]),
        'gfft_ps_rk_stage': (c.c_int, [vp, vp, vp, vp, c.c_int64, c.c_double, c.c_double, c.c_int, vp]),
        'gfft_ps_spectrum': (c.c_int, [vp, c.c_int, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double, c.c_int,
                                       vp, c.c_int, vp]),
        'gfft_ps_cospectrum': (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_double, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64,
                                         c.c_double, c.c_int, vp, c.c_int, vp]),
        'gfft_ps_stats': (c.c_int, [vp, c.c_int, c.c_int64, c.POINTER(c.c_double), vp, c.c_int, vp]),
        'gfft_ps_timestep': (c.c_int, [vp, c.c_double, c.c_double, c.c_double, vp, vp]),
        'gfft_ps_rk_stage_dt': (c.c_int, [vp, vp, vp, vp, c.c_int64, c.c_double, c.c_double, vp, c.c_int, vp]),
        'gfft_ps_force_gain': (c.c_int, [vp, c.c_int, c.c_int, c.c_int, c.c_double, c.c_double, vp, vp]),
        'gfft_ps_project_forced': (c.c_int, [vp, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double, c.c_double,
                                             c.c_int, c.c_int, c.c_double, vp, c.c_int, vp]),
        'gfft_ps_project_dealiased': (c.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double,
                                                c.c_double, c.c_int, c.c_double, c.c_int, c.c_int, c.c_double, vp, c.c_int, vp]),
        'gfft_ps_dealias': (c.c_int, [vp, c.c_int, vp, vp, vp, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double,
                                      c.c_int, vp]),
        'gfft_ps_scalar_flux': (c.c_int, [vp, vp, vp, c.c_int, c.c_int64, c.c_int, vp]),
        'gfft_ps_scalar_rhs': (c.c_int, [vp, vp, vp, vp, c.c_int, c.POINTER(c.c_double), c.POINTER(c.c_double), vp, vp, vp,
                                         vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_double, c.c_int, vp]),
        'gfft_ps_rk_stage_if': (c.c_int, [vp, vp, vp, vp, c.c_int, c.POINTER(c.c_double), vp, vp, vp, c.c_int64, c.c_int64, c.c_int64,
                                          c.c_double, c.c_double, c.c_int, c.c_int, c.c_int, c.c_int, c.c_double, vp, c.c_int, vp]),
        'gfft_ps_gradient': (c.c_int, [vp, vp, c.c_int, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_int, vp]),
        'gfft_ps_gradient_stats': (c.c_int, [vp, c.c_int64, vp, c.c_int, vp]),
        'gfft_ps_structure': (c.c_int, [vp, c.c_int, i64p, c.c_int, c.c_int, c.POINTER(c.c_int32), c.c_int, vp, c.c_int, vp]),
        'gfft_ps_histogram': (c.c_int, [vp, c.c_int, c.c_int64, c.POINTER(c.c_double), c.POINTER(c.c_double), c.c_int, vp,
                                        c.c_int, vp]),
        'gfft_ps_gradient_pdf': (c.c_int, [vp, c.c_int64, c.c_int, c.c_double, c.c_double, c.c_int, c.c_int, c.c_double,
                                           c.c_double, c.c_int, vp, c.c_int, vp]),
        'gfft_ps_scale_axes': (c.c_int, [vp, vp, c.c_int, vp, vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_int, vp]),
        'gfft_ps_interp': (c.c_int, [vp, c.c_int, i64p, i64p, i64p, c.POINTER(c.c_double), vp, c.c_int64, c.c_int, vp, c.c_int, vp]),
        'gfft_ps_spread': (c.c_int, [vp, c.c_int, i64p, i64p, i64p, c.POINTER(c.c_double), vp, vp, c.c_int64, c.c_int, c.c_int, vp, vp]),
        'gfft_ps_spread_finish': (c.c_int, [vp, vp, c.c_int64, c.c_double, c.c_int, c.c_int, vp]),
        'gfft_ps_random_field': (c.c_int, [vp, c.c_int, i64p, i64p, i64p, vp, vp, vp, c.c_int, c.c_double, vp, c.c_int, c.c_uint64,
                                           c.c_uint64, c.c_int, c.c_int, vp]),
        'gfft_ps_scale_shells': (c.c_int, [vp, vp, c.c_int, vp, vp, vp, c.c_double, vp, c.c_int, c.c_int64, c.c_int64, c.c_int64,
                                           c.c_int, vp]),
        'gfft_debug_pass': (c.c_int, [i64p, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp]),
        'gfft_malloc': (c.c_int, [c.POINTER(vp), c.c_size_t]),
        'gfft_free': (c.c_int, [vp]),
        'gfft_memcpy_h2d': (c.c_int, [vp, vp, c.c_size_t, vp]),
        'gfft_memcpy_d2h': (c.c_int, [vp, vp, c.c_size_t, vp]),
        'gfft_memcpy_d2d': (c.c_int, [vp, vp, c.c_size_t, vp]),
        'gfft_stream_synchronize': (c.c_int, [vp]),
        'gfft_event_create': (c.c_int, [c.POINTER(vp)]),
        'gfft_event_record': (c.c_int, [vp, vp]),
        'gfft_event_elapsed_ms': (c.c_int, [vp, vp, c.POINTER(c.c_float)]),
        'gfft_event_destroy': (c.c_int, [vp]),
        'gfft_plan_profile': (c.c_int, [vp, c.POINTER(c.c_float), c.c_int, ip]),
        'gfft_plan_pass_info': (c.c_int, [vp, c.c_int, c.c_char_p, c.c_size_t, c.POINTER(c.c_double)]),
        'gfft_plan_pass_launch': (c.c_int, [vp, c.c_int, i64p, ip]),
        'gfft_probe_copy': (c.c_int, [vp, vp, c.c_size_t, vp]),
        'gfft_async_error': (c.c_int, []),
        'gfft_plan_status': (c.c_int, [vp]),
        'gfft_rccl_load': (c.c_int, [c.c_char_p]),
        'gfft_rccl_info': (c.c_int, [c.c_char_p, c.c_size_t]),
        'gfft_exchange_last_error': (c.c_char_p, []),
        'gfft_comm_get_unique_id': (c.c_int, [vp]),
        'gfft_comm_create': (c.c_int, [c.POINTER(vp), vp, c.c_int, c.c_int]),
        'gfft_comm_split': (c.c_int, [vp, c.c_int, c.c_int, c.POINTER(vp)]),
        'gfft_comm_rank': (c.c_int, [vp, ip, ip]),
        'gfft_comm_destroy': (c.c_int, [vp]),
        'gfft_sendrecv': (c.c_int, [vp, c.c_int, c.POINTER(Msg), c.c_int, c.POINTER(Msg), vp]),
        'gfft_alltoallv': (c.c_int, [vp, vp, i64p, i64p, vp, i64p, i64p, c.c_int, vp]),
        'gfft_stream_create': (c.c_int, [c.POINTER(vp)]),
        'gfft_stream_destroy': (c.c_int, [vp]),
        'gfft_stream_wait_event': (c.c_int, [vp, vp]),
        'gfft_event_create_untimed': (c.c_int, [c.POINTER(vp)]),
        'gfft_probe_tile_copy': (c.c_int, [vp, vp, c.c_int64, c.c_int64, c.c_int64, c.c_int, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sigs


EXPORTS = None


def lib():
    """The loaded shared library; raises if it has not been built."""
    global _lib, EXPORTS
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise ImportError(
                "libgfft.so is not built (%s). Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C mpi4py-fft_amd/csrc`. There is no CPU fallback." % LIBPATH)
        _lib = ctypes.CDLL(LIBPATH)
        EXPORTS = _declare(_lib)
    return _lib


def check_async():
    """Raise if a launch that already returned has failed since the last look (gfft_async_error: a fused pass pair
    that gave up a wait).  Called where the host is about to READ results, after the synchronisation."""
    if _lib is not None:
        check(_lib.gfft_async_error())


def check(rc):
    if rc != 0:
        l = lib()
        detail = l.gfft_last_error().decode() or l.gfft_exchange_last_error().decode()
        raise GfftError('%s: %s' % (l.gfft_strerror(rc).decode(), detail))


def check_wire(rc):
    """status of an exchange-module call (its error text is kept separately from the planner's)"""
    if rc != 0:
        l = lib()
        raise GfftError('%s: %s' % (l.gfft_strerror(rc).decode(), l.gfft_exchange_last_error().decode()))


def _i64(seq):
    return (ctypes.c_int64 * len(seq))(*[int(s) for s in seq])


_raw_stream = None


def current_stream():
    """hipStream_t of torch's current stream (torch owns device memory and streams here).
    Uses torch's raw-handle accessor when it exists: the public `current_stream()` builds a Stream
    object per call, ~7 us of the ~16 us a small transform costs on the host."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        fast = getattr(torch._C, '_cuda_getCurrentRawStream', None)
        if fast is not None and torch.cuda.is_available():
            _raw_stream = lambda: ctypes.c_void_p(fast(torch.cuda.current_device()))
        elif torch.cuda.is_available():
            _raw_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        else:
            _raw_stream = lambda: ctypes.c_void_p(0)
    return _raw_stream()


def precision_of(dtype):
    return 8 if np.dtype(dtype).char in 'dD' else 4


class HipEngine:
    """The product engine: every method is one call through the C ABI."""
    name = 'hip'

    def require_device(self, tensor):
        if tensor.device.type != 'cuda':
            raise GfftError('array lives on %s: libgfft runs on HIP device memory only '
                            '(no CPU fallback)' % tensor.device)

    def plan_create(self, sizes_in, sizes_out, axes, kind, precision):
        h = ctypes.c_void_p()
        ax = (ctypes.c_int * len(axes))(*[int(a) for a in axes])
        check(lib().gfft_plan_create(ctypes.byref(h), len(sizes_in), _i64(sizes_in), _i64(sizes_out),
                                     len(axes), ax, int(kind), int(precision)))
        return h

    def plan_create_r2r(self, sizes, axes, kinds, precision):
        h = ctypes.c_void_p()
        ax = (ctypes.c_int * len(axes))(*[int(a) for a in axes])
        kd = (ctypes.c_int * len(kinds))(*[int(k) for k in kinds])
        check(lib().gfft_plan_create_r2r(ctypes.byref(h), len(sizes), _i64(sizes), len(axes), ax, kd,
                                         int(precision)))
        return h

    def plan_create_guru(self, precision, kind, dim, howmany, in_blocks=1, in_block_stride=0, out_blocks=1,
                         out_block_stride=0, n_keep=0):
        """Strided batched 1-D plan (gfft_plan_create_guru); dim / howmany entries are (n, is, os).
        n_keep: entries kept on the truncated side of a fused 3/2-rule truncation / zero padding
        (gfft_plan_create_guru_padded).  None when the engine has no single-pass kernel for it."""
        h = ctypes.c_void_p()
        hm = (IoDim * max(1, len(howmany)))(*[IoDim(*[int(x) for x in d]) for d in howmany])
        rc = lib().gfft_plan_create_guru_padded(ctypes.byref(h), int(precision), int(kind), ctypes.byref(IoDim(*[int(x) for x in dim])),
                                                int(n_keep), len(howmany), hm, int(in_blocks), int(in_block_stride),
                                                int(out_blocks), int(out_block_stride))
        if rc == -2:
            return None
        check(rc)
        return h

    def plan_create_guru2(self, precision, kind, cols, rows, planes, cols_first=False, in_blocks=1, in_block_stride=0,
                          out_blocks=1, out_block_stride=0):
        """Batched 2-D plan, plane by plane, as ONE launch where a fused pair exists (gfft_plan_create_guru2): the two
        local stages of a slab-decomposed transform.  cols / rows / planes are (n, is, os).  None when the engine has
        no single-pass kernels for the lengths; `plan_cost(h)[2]` tells whether it runs as one launch or two."""
        h = ctypes.c_void_p()
        io = lambda d: ctypes.byref(IoDim(*[int(x) for x in d]))
        rc = lib().gfft_plan_create_guru2(ctypes.byref(h), int(precision), int(kind), io(cols), io(rows), io(planes),
                                          1 if cols_first else 0, int(in_blocks), int(in_block_stride), int(out_blocks),
                                          int(out_block_stride))
        if rc == -2:
            return None
        check(rc)
        return h

    def plan_create_guru2_real(self, precision, kind, cols, rows, planes, in_blocks=1, in_block_stride=0, out_blocks=1,
                               out_block_stride=0):
        """plan_create_guru2 for real planes (gfft_plan_create_guru2_real): kind R2C = [r2c rows -> strided], C2R = [strided ->
        c2r rows]; rows[0] is the real length; strides in reals on the real side, complex entries on the half-spectrum side,
        blocks on the half-spectrum side only.  None when the engine has no single-pass kernels for it; `plan_cost(h)[2]`
        tells whether it runs as one launch or two."""
        h = ctypes.c_void_p()
        io = lambda d: ctypes.byref(IoDim(*[int(x) for x in d]))
        rc = lib().gfft_plan_create_guru2_real(ctypes.byref(h), int(precision), int(kind), io(cols), io(rows), io(planes),
                                               int(in_blocks), int(in_block_stride), int(out_blocks), int(out_block_stride))
        if rc == -2:
            return None
        check(rc)
        return h

    def execute_ptr(self, h, ptr_in, ptr_out, scale, stream=None):
        """gfft_execute on raw device addresses (element 0 of the plan's input / output)."""
        check(lib().gfft_execute(h, ctypes.c_void_p(ptr_in), ctypes.c_void_p(ptr_out), float(scale),
                                 current_stream() if stream is None else stream))

    def plan_status(self, h):
        """gfft_plan_status: raises if a launch of THIS plan voided itself since anybody last looked (call after a sync)."""
        check(lib().gfft_plan_status(h))

    def plan_execute(self, h, tin, tout, scale):
        self.require_device(tin)
        self.require_device(tout)
        check(lib().gfft_execute(h, tin.data_ptr(), tout.data_ptr(), float(scale), current_stream()))

    def plan_create_padded(self, padded, kept, kind, precision):
        """The padded 3-D transform of a one-rank PFFT as one plan, or None when libgfft keeps the
        per-axis form (gfft_plan_create_padded)."""
        h = ctypes.c_void_p()
        rc = lib().gfft_plan_create_padded(ctypes.byref(h), _i64(padded), _i64(kept), int(kind), int(precision))
        if rc == -2:
            return None
        check(rc)
        return h

    def plan_set_truncation(self, h, n_keep):
        """True if the truncation/padding was fused into the plan, False if it cannot be."""
        rc = lib().gfft_plan_set_truncation(h, int(n_keep))
        if rc == -2:
            return False
        check(rc)
        return True

    def plan_set_split(self, h, side, nblocks):
        """Packed (all-to-all buffer) layout on the plan's input (side 0) / output (side 1);
        True if fused, False if this plan cannot (caller keeps the pack / unpack kernel)."""
        rc = lib().gfft_plan_set_split(h, int(side), int(nblocks))
        if rc == -2:
            return False
        check(rc)
        return True

    def plan_set_tiles(self, h, side, tile, tile_stride):
        """Tile-major exchange-buffer layout on one side of a one-pass plan (gfft_plan_set_tiles);
        False if the plan's kernel cannot address it."""
        rc = lib().gfft_plan_set_tiles(h, int(side), int(tile), int(tile_stride))
        if rc == -2:
            return False
        check(rc)
        return True

    def plan_set_flat(self, h, body_width=0, tail_offset=0, tail_row_stride=0):
        """Tiles over the flattened batch dims of a strided plan, optionally reading rows stored as
        body + leftover columns (gfft_plan_set_flat)."""
        rc = lib().gfft_plan_set_flat(h, int(body_width), int(tail_offset), int(tail_row_stride))
        if rc == -2:
            return False
        check(rc)
        return True

    def plan_set_split_slabs(self, h, side, nblocks, rows_per_slab, tile):
        """gfft_plan_set_split_slabs: uneven blocks of packed-real rows, slab by slab, tile-major."""
        rc = lib().gfft_plan_set_split_slabs(h, int(side), int(nblocks), int(rows_per_slab), int(tile))
        if rc == -2:
            return False
        check(rc)
        return True

    def plan_destroy(self, h):
        if h is not None and _lib is not None:
            _lib.gfft_plan_destroy(h)

    def plan_describe(self, h):
        buf = ctypes.create_string_buffer(4096)
        check(lib().gfft_plan_describe(h, buf, 4096))
        return buf.value.decode()

    def plan_cost(self, h):
        f, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        check(lib().gfft_plan_cost(h, ctypes.byref(f), ctypes.byref(b), ctypes.byref(n)))
        return f.value, b.value, n.value

    def plan_profile(self, h, npasses):
        """[(kernel family, algorithmic bytes per launch, total ms, launches)] per pass since the
        last call; needs set_option('profile', 1) during the executes."""
        ms = (ctypes.c_float * npasses)()
        n = ctypes.c_int()
        check(lib().gfft_plan_profile(h, ms, npasses, ctypes.byref(n)))
        out = []
        for i in range(npasses):
            buf = ctypes.create_string_buffer(64)
            b = ctypes.c_double()
            check(lib().gfft_plan_pass_info(h, i, buf, 64, ctypes.byref(b)))
            out.append((buf.value.decode(), b.value, float(ms[i]), n.value))
        return out

    def plan_pass_launch(self, h):
        """TEST AID (gfft_plan_pass_launch): [(tiles, workgroups)] of every pass's most recent launch, (0, 0) before the first
        execute; raises for a plan with a persistent fused pair."""
        out = []
        for i in range(self.plan_cost(h)[2]):
            t, w = ctypes.c_int64(), ctypes.c_int()
            check(lib().gfft_plan_pass_launch(h, i, ctypes.byref(t), ctypes.byref(w)))
            out.append((t.value, w.value))
        return out

    def pack(self, tarray, tpacked, shape, axis, nparts, itemsize):
        self.require_device(tarray)
        check(lib().gfft_pack(tarray.data_ptr(), tpacked.data_ptr(), len(shape), _i64(shape), axis,
                              nparts, itemsize, current_stream()))

    def unpack(self, tpacked, tarray, shape, axis, nparts, itemsize):
        self.require_device(tarray)
        check(lib().gfft_unpack(tpacked.data_ptr(), tarray.data_ptr(), len(shape), _i64(shape), axis,
                                nparts, itemsize, current_stream()))

    def pack_ptr(self, ptr_array, ptr_packed, shape, axis, nparts, itemsize, unpack=False):
        """gfft_pack / gfft_unpack on raw device addresses (sub-arrays of exchange buffers, pipeline.py)."""
        fn = lib().gfft_unpack if unpack else lib().gfft_pack
        a, b = (ptr_packed, ptr_array) if unpack else (ptr_array, ptr_packed)
        check(fn(ctypes.c_void_p(a), ctypes.c_void_p(b), len(shape), _i64(shape), axis, nparts, itemsize, current_stream()))

    def truncate(self, tpadded, ttrunc, shape_padded, axis, n_trunc, is_real, precision, scale):
        self.require_device(tpadded)
        check(lib().gfft_truncate(tpadded.data_ptr(), ttrunc.data_ptr(), len(shape_padded),
                                  _i64(shape_padded), axis, n_trunc, int(is_real), precision,
                                  float(scale), current_stream()))

    def pad(self, ttrunc, tpadded, shape_padded, axis, n_trunc, is_real, precision):
        self.require_device(tpadded)
        check(lib().gfft_pad(ttrunc.data_ptr(), tpadded.data_ptr(), len(shape_padded),
                             _i64(shape_padded), axis, n_trunc, int(is_real), precision,
                             current_stream()))

    def scale(self, t, count, precision, scale):
        self.require_device(t)
        check(lib().gfft_scale(t.data_ptr(), count, precision, float(scale), current_stream()))

    # pseudo-spectral caller kernels (spectral.py)
    def ps_curl(self, tu, tout, k, shape, precision):
        self.require_device(tu)
        check(lib().gfft_ps_curl(tu.data_ptr(), tout.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                 shape[0], shape[1], shape[2], precision, current_stream()))

    def ps_cross(self, ta, tb, tout, count, precision):
        self.require_device(ta)
        check(lib().gfft_ps_cross(ta.data_ptr(), tb.data_ptr(), tout.data_ptr(), count, precision, current_stream()))

    def ps_project(self, tdu, tu, k, shape, nu, precision):
        self.require_device(tdu)
        check(lib().gfft_ps_project(tdu.data_ptr(), tu.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                    shape[0], shape[1], shape[2], float(nu), precision, current_stream()))

    def ps_rk_stage(self, tu, tu0, tu1, tdu, count, cb, ca, precision):
        self.require_device(tu1)
        check(lib().gfft_ps_rk_stage(None if tu is None else tu.data_ptr(), None if tu0 is None else tu0.data_ptr(),
                                     tu1.data_ptr(), tdu.data_ptr(), count, float(cb), float(ca), precision,
                                     current_stream()))

    def ps_spectrum(self, tu, ncomp, k, w2, shape, dk, nbins, tout, precision):
        """gfft_ps_spectrum: tout = double[2][nbins] on the device, overwritten; w2 None = weight 1."""
        self.require_device(tu)
        self.require_device(tout)
        check(lib().gfft_ps_spectrum(tu.data_ptr(), int(ncomp), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                     None if w2 is None else w2.data_ptr(), shape[0], shape[1], shape[2], float(dk),
                                     int(nbins), tout.data_ptr(), precision, current_stream()))

    def ps_cospectrum(self, ta, tb, ncomp, op, scale, k, w2, shape, dk, nbins, tout, precision):
        """gfft_ps_cospectrum: op = PS_DOT / PS_HELICITY (tb None); tout = double[2][nbins] on the device, overwritten."""
        self.require_device(ta)
        self.require_device(tout)
        if tb is not None:
            self.require_device(tb)
        check(lib().gfft_ps_cospectrum(ta.data_ptr(), None if tb is None else tb.data_ptr(), int(ncomp), int(op), float(scale),
                                       k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                       None if w2 is None else w2.data_ptr(), shape[0], shape[1], shape[2], float(dk),
                                       int(nbins), tout.data_ptr(), precision, current_stream()))

    def ps_stats(self, tu, ncomp, count, inv_dx, tout, precision):
        """gfft_ps_stats: tu = real [ncomp][count]; inv_dx = ncomp host floats; tout = double[2 + 6 ncomp] on the device,
        overwritten."""
        self.require_device(tu)
        self.require_device(tout)
        inv = (ctypes.c_double * int(ncomp))(*[float(x) for x in inv_dx])
        check(lib().gfft_ps_stats(tu.data_ptr(), int(ncomp), int(count), inv, tout.data_ptr(), precision, current_stream()))

    def ps_timestep(self, tstats, cfl, dt_min, dt_max, tdt):
        """gfft_ps_timestep: tdt = double[2] on the device: [0] = the clamped step, [1] += it."""
        self.require_device(tstats)
        self.require_device(tdt)
        check(lib().gfft_ps_timestep(tstats.data_ptr(), float(cfl), float(dt_min), float(dt_max), tdt.data_ptr(),
                                     current_stream()))

    def ps_rk_stage_dt(self, tu, tu0, tu1, tdu, count, cb, ca, tdt, precision):
        """gfft_ps_rk_stage_dt: ps_rk_stage with the coefficients cb * tdt[0], ca * tdt[0] (tdt: device double)."""
        self.require_device(tu1)
        self.require_device(tdt)
        check(lib().gfft_ps_rk_stage_dt(None if tu is None else tu.data_ptr(), None if tu0 is None else tu0.data_ptr(),
                                        tu1.data_ptr(), tdu.data_ptr(), count, float(cb), float(ca), tdt.data_ptr(),
                                        precision, current_stream()))

    def ps_force_gain(self, tspec, nbins, blo, bhi, eps, gain_max, tgain):
        """gfft_ps_force_gain: tspec = double[2][nbins] as ps_spectrum writes it; tgain = double[2] on the device:
        [0] = min(eps / (2 E_f), gain_max), [1] = E_f, the energy of shells blo..bhi."""
        self.require_device(tspec)
        self.require_device(tgain)
        check(lib().gfft_ps_force_gain(tspec.data_ptr(), int(nbins), int(blo), int(bhi), float(eps), float(gain_max),
                                       tgain.data_ptr(), current_stream()))

    def ps_project_forced(self, tdu, tu, k, shape, nu, dk, blo, bhi, gain, tgain, precision):
        """gfft_ps_project_forced: ps_project, then du += g u in shells blo..bhi; g = tgain[0] (device double) or, tgain
        None, the float `gain`."""
        self.require_device(tdu)
        if tgain is not None:
            self.require_device(tgain)
        check(lib().gfft_ps_project_forced(tdu.data_ptr(), tu.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                           shape[0], shape[1], shape[2], float(nu), float(dk), int(blo), int(bhi),
                                           float(gain), None if tgain is None else tgain.data_ptr(), precision,
                                           current_stream()))

    def ps_project_dealiased(self, tdu, tu, k, m, shape, nu, kcut, force, precision):
        """gfft_ps_project_dealiased: ps_project (force None) or ps_project_forced (force = (dk, blo, bhi, gain, tgain) as
        there), keeping the modes with m[0][i0] && m[1][i1] && m[2][i2] (uint8 device vectors; None = the whole axis) and
        |k| <= kcut (inf: no spherical cut); every other mode of tdu becomes +0 and is not read."""
        self.require_device(tdu)
        dk, blo, bhi, gain, tgain = (1.0, 0, 0, 0.0, None) if force is None else force
        for t in tuple(m) + (tgain,):
            if t is not None:
                self.require_device(t)
        check(lib().gfft_ps_project_dealiased(tdu.data_ptr(), tu.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                              *[None if t is None else t.data_ptr() for t in m],
                                              shape[0], shape[1], shape[2], float(nu), float(kcut), 0 if force is None else 1,
                                              float(dk), int(blo), int(bhi), float(gain),
                                              None if tgain is None else tgain.data_ptr(), precision, current_stream()))

    def ps_dealias(self, tf, ncomp, k, m, shape, kcut, precision):
        """gfft_ps_dealias: +0 to every truncated mode of tf = complex [ncomp] + shape, in place; kept modes are not touched.
        m and kcut as for ps_project_dealiased."""
        self.require_device(tf)
        for t in m:
            if t is not None:
                self.require_device(t)
        check(lib().gfft_ps_dealias(tf.data_ptr(), int(ncomp), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                    *[None if t is None else t.data_ptr() for t in m],
                                    shape[0], shape[1], shape[2], float(kcut), precision, current_stream()))

    def ps_scalar_flux(self, tu, ttheta, tflux, nscalar, count, precision):
        """gfft_ps_scalar_flux: tflux[s][c] = tu[c] * ttheta[s] on real fields of `count` points per component; tflux
        overlaps neither input."""
        for t in (tu, ttheta, tflux):
            self.require_device(t)
        check(lib().gfft_ps_scalar_flux(tu.data_ptr(), ttheta.data_ptr(), tflux.data_ptr(), int(nscalar), int(count), precision,
                                        current_stream()))

    def ps_scalar_rhs(self, tdtheta, tflux, ttheta, tu, nscalar, kappa, grad, k, m, shape, kcut, precision):
        """gfft_ps_scalar_rhs: tdtheta[s] = -i K . tflux[s] - kappa[s] |K|^2 ttheta[s] - grad[s] . tu for nscalar scalars;
        kappa = nscalar host floats, grad = nscalar x 3 host floats or None (tu, which may be None, is then not read);
        m and kcut as for ps_project_dealiased (all None and inf: every mode is kept)."""
        for t in (tdtheta, tflux, ttheta, tu) + tuple(m):
            if t is not None:
                self.require_device(t)
        kap = (ctypes.c_double * int(nscalar))(*[float(x) for x in kappa])
        g = None if grad is None else (ctypes.c_double * (3 * int(nscalar)))(*[float(x) for row in grad for x in row])
        check(lib().gfft_ps_scalar_rhs(tdtheta.data_ptr(), tflux.data_ptr(), ttheta.data_ptr(), None if tu is None else tu.data_ptr(),
                                       int(nscalar), kap, g, k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                       *[None if t is None else t.data_ptr() for t in m],
                                       shape[0], shape[1], shape[2], float(kcut), precision, current_stream()))

    def ps_rk_stage_if(self, tu, tu0, tu1, tdu, ncomp, nu, k, shape, cb, ca, powers, h, tdt, precision):
        """gfft_ps_rk_stage_if: tu = E^q0 tu0 + cb h E^qd tdu (tu None: skipped), tu1 = E^q1 tu1 + ca h E^qa tdu on complex
        [ncomp] + shape, E = exp(-nu[c] |K|^2 h / 2); nu = ncomp host floats, powers = (q0, qd, q1, qa) in 0 ... 2; h = tdt[0]
        (device double) or, tdt None, the float `h`."""
        for t in (tu, tu0, tu1, tdu, tdt):
            if t is not None:
                self.require_device(t)
        v = (ctypes.c_double * int(ncomp))(*[float(x) for x in nu])
        q0, qd, q1, qa = (int(q) for q in powers)
        check(lib().gfft_ps_rk_stage_if(None if tu is None else tu.data_ptr(), None if tu0 is None else tu0.data_ptr(),
                                        tu1.data_ptr(), tdu.data_ptr(), int(ncomp), v, k[0].data_ptr(), k[1].data_ptr(),
                                        k[2].data_ptr(), shape[0], shape[1], shape[2], float(cb), float(ca), q0, qd, q1, qa,
                                        float(h), None if tdt is None else tdt.data_ptr(), precision, current_stream()))

    def ps_gradient(self, tf, tout, ncomp, k, shape, precision):
        """gfft_ps_gradient: tout[c][j] = i k[j] tf[c] on complex tf = [ncomp] + shape, tout = [ncomp][3] + shape; tout overlaps
        nothing."""
        self.require_device(tf)
        self.require_device(tout)
        check(lib().gfft_ps_gradient(tf.data_ptr(), tout.data_ptr(), int(ncomp), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                     shape[0], shape[1], shape[2], precision, current_stream()))

    def ps_gradient_stats(self, ta, count, tout, precision):
        """gfft_ps_gradient_stats: ta = real [3][3][count], ta[i][j] = d u_i / d x_j; tout = double[PS_GRAD_NVAL] on the device,
        overwritten."""
        self.require_device(ta)
        self.require_device(tout)
        check(lib().gfft_ps_gradient_stats(ta.data_ptr(), int(count), tout.data_ptr(), precision, current_stream()))

    def ps_structure(self, tu, ncomp, n, axis, seps, lcomp, tout, precision):
        """gfft_ps_structure: tu = real [ncomp] + n, a block that spans the whole periodic axis `axis`; seps = host integers in
        [0, n[axis]); lcomp = the longitudinal component of the mixed moment or -1; tout = double[len(seps)][ncomp][PS_SF_NVAL]
        on the device, overwritten with the power sums of the increments."""
        self.require_device(tu)
        self.require_device(tout)
        sp = (ctypes.c_int32 * len(seps))(*[int(r) for r in seps])
        check(lib().gfft_ps_structure(tu.data_ptr(), int(ncomp), _i64(n), int(axis), len(seps), sp, int(lcomp), tout.data_ptr(),
                                      precision, current_stream()))

    def ps_random_field(self, tout, ncomp, n, start, N, k, project, dk, tamp, nbins, seed, stream_id, add, precision):
        """gfft_ps_random_field: tout = complex [ncomp] + n, the block start .. start + n of a spectral array over the physical
        grid N, filled with (add: added to by) random modes keyed by their global index; k = the block's three wavenumber
        vectors; tamp = device double[nbins] or None (every amplitude 1); seed below 2^64, stream_id below 2^62."""
        self.require_device(tout)
        if tamp is not None:
            self.require_device(tamp)
        check(lib().gfft_ps_random_field(tout.data_ptr(), int(ncomp), _i64(n), _i64(start), _i64(N), k[0].data_ptr(), k[1].data_ptr(),
                                         k[2].data_ptr(), int(bool(project)), float(dk), None if tamp is None else tamp.data_ptr(),
                                         int(nbins), int(seed), int(stream_id), int(bool(add)), precision, current_stream()))

    def ps_scale_shells(self, tf, tout, ncomp, k, dk, ttab, nbins, shape, precision):
        """gfft_ps_scale_shells: tout[c] = tf[c] * (real)ttab[shell] on complex [ncomp] + shape, +0 where the shell is >= nbins;
        ttab = device double[nbins]; tout is tf or overlaps nothing."""
        self.require_device(tf)
        self.require_device(tout)
        self.require_device(ttab)
        check(lib().gfft_ps_scale_shells(tout.data_ptr(), tf.data_ptr(), int(ncomp), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                         float(dk), ttab.data_ptr(), int(nbins), shape[0], shape[1], shape[2], precision,
                                         current_stream()))

    def ps_histogram(self, tu, ncomp, count, lo, hi, nbins, tout, precision):
        """gfft_ps_histogram: tu = real [ncomp][count]; lo, hi = ncomp host floats each; tout = int64[ncomp][nbins + PS_PDF_TAIL]
        on the device, overwritten."""
        self.require_device(tu)
        self.require_device(tout)
        los = (ctypes.c_double * int(ncomp))(*[float(x) for x in lo])
        his = (ctypes.c_double * int(ncomp))(*[float(x) for x in hi])
        check(lib().gfft_ps_histogram(tu.data_ptr(), int(ncomp), int(count), los, his, int(nbins), tout.data_ptr(), precision,
                                      current_stream()))

    def ps_gradient_pdf(self, ta, count, qx, xr, nbx, qy, yr, nby, tout, precision):
        """gfft_ps_gradient_pdf: ta = real [3][3][count]; qx, qy among PS_Q_* (qy = PS_Q_NONE: the 1-D table of qx, nby = 1);
        xr, yr = (lo, hi); tout = int64[nbx + PS_PDF_TAIL] or int64[nbx * nby + 2] on the device, overwritten."""
        self.require_device(ta)
        self.require_device(tout)
        check(lib().gfft_ps_gradient_pdf(ta.data_ptr(), int(count), int(qx), float(xr[0]), float(xr[1]), int(nbx), int(qy),
                                         float(yr[0]), float(yr[1]), int(nby), tout.data_ptr(), precision, current_stream()))

    def ps_scale_axes(self, tf, tout, ncomp, v, shape, precision):
        """gfft_ps_scale_axes: tout[c] = tf[c] * (v[0][i0] * v[1][i1]) * v[2][i2] on complex [ncomp] + shape; v = three real
        device vectors of the field's precision or None (no factor from that axis); tout is tf or overlaps nothing."""
        self.require_device(tf)
        self.require_device(tout)
        for vi in v:
            if vi is not None:
                self.require_device(vi)
        check(lib().gfft_ps_scale_axes(tout.data_ptr(), tf.data_ptr(), int(ncomp), *[None if vi is None else vi.data_ptr() for vi in v],
                                       shape[0], shape[1], shape[2], precision, current_stream()))

    def ps_interp(self, tc, ncomp, n, start, N, inv_dx, tx, npart, order, tout, precision):
        """gfft_ps_interp: tc = real [ncomp] + n, the block start .. start + n of a periodic grid N; inv_dx = three host floats;
        tx = double [npart][3]; tout = double [npart][ncomp] on the device, overwritten with this block's share of the
        order-2 or order-4 interpolant."""
        self.require_device(tc)
        self.require_device(tx)
        self.require_device(tout)
        dx = (ctypes.c_double * 3)(*[float(d) for d in inv_dx])
        check(lib().gfft_ps_interp(tc.data_ptr(), int(ncomp), _i64(n), _i64(start), _i64(N), dx, tx.data_ptr(), int(npart), int(order),
                                   tout.data_ptr(), precision, current_stream()))

    def ps_spread(self, tacc, ncomp, n, start, N, inv_dx, tx, tq, npart, order, scale_exp, tskipped):
        """gfft_ps_spread: tacc = int64 [ncomp] + n, ADDED to with this block's share of the particles' contributions in fixed
        point (2^scale_exp units per unit of q); tx = double [npart][3], tq = double [npart][ncomp]; tskipped = int64 [1], grows
        by the number of particles that are not finite or too large."""
        for t in (tacc, tx, tq, tskipped):
            self.require_device(t)
        dx = (ctypes.c_double * 3)(*[float(d) for d in inv_dx])
        check(lib().gfft_ps_spread(tacc.data_ptr(), int(ncomp), _i64(n), _i64(start), _i64(N), dx, tx.data_ptr(), tq.data_ptr(), int(npart),
                                   int(order), int(scale_exp), tskipped.data_ptr(), current_stream()))

    def ps_spread_finish(self, tout, tacc, count, factor, clear, precision):
        """gfft_ps_spread_finish: tout[i] = (real)((double)tacc[i] * factor) over count values, then tacc[i] = 0 where clear"""
        self.require_device(tout)
        self.require_device(tacc)
        check(lib().gfft_ps_spread_finish(tout.data_ptr(), tacc.data_ptr(), int(count), float(factor), int(bool(clear)), precision,
                                          current_stream()))

    def copy(self, tsrc, tdst):
        self.require_device(tsrc)
        check(lib().gfft_memcpy_d2d(tdst.data_ptr(), tsrc.data_ptr(),
                                    tsrc.numel() * tsrc.element_size(), current_stream()))


_engine = HipEngine()


def engine():
    return _engine


def set_engine(e):
    """TEST SEAM ONLY (see module docstring).  Returns the previous engine."""
    global _engine
    old, _engine = _engine, (e if e is not None else HipEngine())
    return old


def set_option(key, value):
    check(lib().gfft_set_option(key.encode(), int(value)))


def device_count():
    n = ctypes.c_int(0)
    rc = lib().gfft_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0
