"""Case list for the tests of csrc/upfirdn2d.hip's dispatcher (launch_up) and of the transposed configuration of
torch_utils/ops/upfirdn2d.py: the filters, the calls, the kernel each call is expected to reach, and float64 references
computed once and shared (read-only) by tests/test_upfirdn2d_cases_cpu.py and tests/test_upfirdn2d_routes_gpu.py.

No test functions here.  Every filter is NON-symmetric, so that a swapped tap order or a wrong flip in the transposed
configuration changes the result; every call is made with flip_filter False and True and with gain 1.7 (not a power of two,
not exact in float32)."""

import collections
import functools
import zlib

import numpy as np

GAIN = 1.7
FLIPS = (False, True)
TOL = {'float32': 2e-5, 'float16': 6e-3, 'float64': 1e-11}       # rtol = tol, atol = tol * max(1, max |ref|)

# ---- what the kernels' geometry is, restated from csrc/upfirdn2d.hip (tests/test_upfirdn2d_cases_cpu.py holds the cases to it:
# retune a tile there and that test names the cases to enlarge)
# Fir4Shape (csrc/upfirdn2d.hip:166-171): OPL = 16 / sizeof(T), CS = OPL * DOWN / UP, LXN = 4 | 8 | 16 lanes across,
# TW = LXN * OPL, TH = 256 / LXN
FIR4_TILE = {('up2', 'float32'): (64, 16), ('up2', 'float16'): (128, 16),
             ('down2', 'float32'): (32, 32), ('down2', 'float16'): (32, 64)}            # (TW, TH)
TILE_TILE = (64, 16)                                # TILE_W, TILE_H (csrc/upfirdn2d.hip:83)
TILE_MAX_TAPS = 8                                   # MAX_TAPS (csrc/upfirdn2d.hip:84); launch_up's `small` also asks down <= 2 (:833)
ANY_MAX_LANES = 256 * 16 * 256                      # launch_up caps upfirdn_any_kernel's grid at kNumCU * 16 blocks (:867) of 256 lanes;
                                                    # kNumCU = 256 (csrc/common.h:61).  More outputs than this: the kernel's loop repeats

KERNELS = ('upfirdn_fir4_kernel', 'upfirdn_tile_kernel', 'upfirdn_any_kernel', 'upfirdn_blur4_kernel', 'upfirdn_blur4_nhwc_kernel')
ROUTE_KERNEL = dict(fir4='upfirdn_fir4_kernel', tile='upfirdn_tile_kernel', any='upfirdn_any_kernel', blur4='upfirdn_blur4_kernel',
                    blur4_nhwc='upfirdn_blur4_nhwc_kernel')

# ---- filters (float32).  The seed is one for which every case meets test_cases_discriminate (tests/test_upfirdn2d_cases_cpu.py) with
# room: with up = 3 and 4 x 3 taps an output is one or two products, so two taps of a flip pair that happen to lie close together
# leave the flip invisible on half of the outputs.  0.73 of the outputs is the weakest figure with this seed (tile_up3_down2, flip).
_frng = np.random.default_rng(102)
FILTERS = {
    'f44': _frng.standard_normal((4, 4)).astype(np.float32),
    'f43': _frng.standard_normal((4, 3)).astype(np.float32),
    'f5': _frng.standard_normal(5).astype(np.float32),              # 1-D: separable, applied as a row pass and a column pass
    'f8': _frng.standard_normal(8).astype(np.float32),
    'f12': _frng.standard_normal(12).astype(np.float32),
}
for _f in FILTERS.values():
    _f.setflags(write=False)

# kind: 'fir4_up2' | 'fir4_down2' | 'tile' | 'any' | 'stride' (grid-stride loop of the any kernel) | 'blur'
# seams: the axes along which a fir4 / tile case must cross a tile boundary
# phase: (PX, PY) of the fir4 up = 2 instantiation the forward call launches, else None
Case = collections.namedtuple('Case', 'name kind shape filt up down padding seams phase')


def _c(name, kind, shape, filt, up, down, padding, seams='xy', phase=None):
    return Case(name, kind, shape, filt, up, down, padding, seams, phase)


_UP2 = (1, 2, 23, 77)           # ~46 x 154 outputs; the odd width puts row starts off the 16-byte grid
_DOWN2 = (1, 2, 141, 75)        # ~70 x 37 outputs

CASES = [
    # upfirdn_fir4_kernel, up = 2: the four phases, crops, and padding wider than the filter (border tiles partly in the zeros)
    _c('up2_p00', 'fir4_up2', _UP2, 'f44', 2, 1, [2, 1, 2, 1], phase=(0, 0)),
    _c('up2_p10', 'fir4_up2', _UP2, 'f44', 2, 1, [1, 2, 2, 1], phase=(1, 0)),
    _c('up2_p01', 'fir4_up2', _UP2, 'f44', 2, 1, [2, 1, 3, 0], phase=(0, 1)),
    _c('up2_p11', 'fir4_up2', _UP2, 'f44', 2, 1, [3, 0, 1, 2], phase=(1, 1)),
    _c('up2_p11_crop', 'fir4_up2', _UP2, 'f44', 2, 1, [-1, 2, 3, -2], phase=(1, 1)),
    _c('up2_p00_crop', 'fir4_up2', _UP2, 'f44', 2, 1, [-2, 4, 0, -1], phase=(0, 0)),
    _c('up2_widepad', 'fir4_up2', _UP2, 'f44', 2, 1, [5, 4, 6, 7], phase=(1, 0)),
    # upfirdn_fir4_kernel, down = 2
    _c('down2_1111', 'fir4_down2', _DOWN2, 'f44', 1, 2, [1, 1, 1, 1]),
    _c('down2_0211', 'fir4_down2', _DOWN2, 'f44', 1, 2, [0, 2, 1, 1]),
    _c('down2_2030', 'fir4_down2', _DOWN2, 'f44', 1, 2, [2, 0, 3, 0]),
    _c('down2_crop', 'fir4_down2', _DOWN2, 'f44', 1, 2, [-1, 2, 0, -3]),
    _c('down2_widepad', 'fir4_down2', _DOWN2, 'f44', 1, 2, [5, 6, 4, 7]),
    # upfirdn_tile_kernel
    _c('tile_wide', 'tile', (2, 2, 19, 150), 'f43', [2, 1], [1, 2], [1, 2, 3, 0], seams='x'),         # 301 wide: 5 tiles across
    _c('tile_tall', 'tile', (1, 2, 40, 70), 'f43', [1, 2], [2, 1], [-1, 3, 2, -2], seams='y'),        # 77 high: 5 tiles down
    _c('tile_sep8_down2', 'tile', (1, 2, 37, 140), 'f8', 1, 2, [4, 3, 5, 2]),                         # two 1-D passes
    _c('tile_sep5_up2', 'tile', (1, 2, 21, 90), 'f5', 2, 1, [3, 2, -1, 4]),                           # 181 wide
    _c('tile_up3_down2', 'tile', (1, 1, 12, 50), 'f43', 3, 2, [2, 2, 1, 3]),                          # an up factor fir4 does not take
    # upfirdn_any_kernel
    _c('any_down3', 'any', (1, 2, 60, 200), 'f8', 2, 3, [4, 3, 5, 2]),
    _c('any_taps12', 'any', (1, 1, 30, 40), 'f12', 4, 1, [10, 9, 8, 11]),
    _c('stride_f64', 'stride', (1, 3, 300, 300), 'f44', 2, 1, [2, 1, 2, 1]),                          # 1,080,000 outputs
    _c('stride_f16_nhwc', 'stride', (1, 8, 190, 190), 'f44', 2, 1, [2, 1, 2, 1]),                     # 1,155,200 outputs
    # the streaming blurs, NCHW and channels_last, over several strips
    _c('blur', 'blur', (1, 16, 70, 33), 'f44', 1, 1, [0, 3, 3, 0]),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FIR4 = [c for c in CASES if c.kind in ('fir4_up2', 'fir4_down2')]
TILE = [c for c in CASES if c.kind == 'tile']
PHASES = [c for c in CASES if c.name in ('up2_p00', 'up2_p10', 'up2_p01', 'up2_p11')]
SECOND_ORDER = PHASES + [BY_NAME['down2_0211'], BY_NAME['down2_crop']]


def runs(case):
    """[(dtype name, layout)] the case is run in; layout is 'nchw' or 'nhwc' (channels_last memory)."""
    if case.name == 'stride_f64':
        return [('float64', 'nchw')]
    if case.name == 'stride_f16_nhwc':
        return [('float16', 'nhwc')]
    if case.kind == 'blur':
        return [(d, lay) for lay in ('nchw', 'nhwc') for d in ('float32', 'float16')]
    nchw = [(d, 'nchw') for d in ('float32', 'float16', 'float64')]
    if case.kind in ('fir4_up2', 'fir4_down2'):
        return nchw + [(d, 'nhwc') for d in ('float32', 'float16', 'float64')]
    return nchw


FORWARD_RUNS = [(c.name, d, lay) for c in CASES for d, lay in runs(c)]


def expected_route(case, dtype, layout):
    """The key of ROUTE_KERNEL that launch_up (csrc/upfirdn2d.hip:829-871) is expected to take for this call."""
    if case.kind == 'blur' and dtype != 'float64':
        return 'blur4' if layout == 'nchw' else 'blur4_nhwc'
    if dtype == 'float64' or layout == 'nhwc' or case.kind in ('any', 'stride'):
        return 'any'
    return 'tile' if case.kind == 'tile' else 'fir4'


def xy(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(in_size, up, down, pad0, pad1, taps):
    return (in_size * up + pad0 + pad1 - taps + down) // down


def launches(case):
    """[(out_h, out_w)] of each kernel launch of the forward call: one for a 2-D filter, row pass then column pass for a 1-D one."""
    f = FILTERS[case.filt]
    (upx, upy), (downx, downy) = xy(case.up), xy(case.down)
    x0, x1, y0, y1 = case.padding
    h, w = case.shape[2:]
    ow = out_size(w, upx, downx, x0, x1, f.shape[-1])
    oh = out_size(h, upy, downy, y0, y1, f.shape[0])
    return [(oh, ow)] if f.ndim == 2 else [(h, ow), (oh, ow)]


def kwargs(case, flip, padding=None):
    return dict(up=case.up, down=case.down, padding=list(case.padding if padding is None else padding), flip_filter=flip, gain=GAIN)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def input64(name, dtype):
    """The case's input: seeded normal values, rounded to the tested dtype and widened to float64."""
    x = _rng(name, 'x').standard_normal(BY_NAME[name].shape)
    return _frozen(x.astype(dtype).astype(np.float64))


@functools.lru_cache(maxsize=None)
def reference(name, flip, dtype, padding=None):
    """oracle.ops_ref.upfirdn2d in float64 on input64(name, dtype); `padding` replaces the case's (a tuple)."""
    from oracle import ops_ref as O
    case = BY_NAME[name]
    return _frozen(O.upfirdn2d(input64(name, dtype), FILTERS[case.filt], **kwargs(case, flip, padding)))


def _torch_form(case, flip, x):
    import torch
    from torch_utils.ops import upfirdn2d
    return upfirdn2d._upfirdn2d_ref(x, torch.from_numpy(FILTERS[case.filt].copy()), **kwargs(case, flip))


def _out_shape(case):
    return tuple(case.shape[:2]) + launches(case)[-1]


@functools.lru_cache(maxsize=None)
def cotangent64(name, dtype):
    """dy: seeded, rounded to the tested dtype, float64."""
    dy = _rng(name, 'dy').standard_normal(_out_shape(BY_NAME[name]))
    return _frozen(dy.astype(dtype).astype(np.float64))


@functools.lru_cache(maxsize=None)
def weight64(name, dtype):
    """w of the second-order test's <dx, w>: seeded, the input's shape."""
    w = _rng(name, 'w').standard_normal(BY_NAME[name].shape)
    return _frozen(w.astype(dtype).astype(np.float64))


@functools.lru_cache(maxsize=None)
def grad_reference(name, flip, dtype):
    """dx = d<op(x), dy>/dx by autograd through _upfirdn2d_ref on float64 CPU tensors."""
    import torch
    x = torch.from_numpy(input64(name, dtype).copy()).requires_grad_(True)
    (dx,) = torch.autograd.grad(_torch_form(BY_NAME[name], flip, x), x, torch.from_numpy(cotangent64(name, dtype).copy()))
    return _frozen(dx.numpy())


@functools.lru_cache(maxsize=None)
def grad2_reference(name, flip, dtype):
    """d<dx, w>/d dy, with dx = d<op(x), dy>/dx built with create_graph, on float64 CPU tensors."""
    import torch
    x = torch.from_numpy(input64(name, dtype).copy()).requires_grad_(True)
    dy = torch.from_numpy(cotangent64(name, dtype).copy()).requires_grad_(True)
    (dx,) = torch.autograd.grad(_torch_form(BY_NAME[name], flip, x), x, dy, create_graph=True)
    (g,) = torch.autograd.grad((dx * torch.from_numpy(weight64(name, dtype).copy())).sum(), dy)
    return _frozen(g.numpy())


def strided_filter(f):
    """The same values and shape with fs_h and fs_w exchanged: a transposed view of the transposed array."""
    return f.t().contiguous().t()
