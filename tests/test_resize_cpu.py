"""CPU tests of the antialiased resize: the float64 restatement (tests/resize_ref.py) against torch, the op's size / scale rules and routes
(torch_utils/ops/resize.py), the C ABI's declarations and refusals, and the two callers."""

import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as R
from torch_utils.ops import resize as RZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (in_size, size, scale_factor): the shapes the restatement was stated for, and the hot ones at full size
TORCH_CASES = {
    'up2_64': ((64, 64), (128, 128), None),
    'down8_512': ((512, 512), (64, 64), None),
    'frac_down_17x13': ((17, 13), (5, 7), None),
    'frac_up_5x7': ((5, 7), (17, 13), None),
    'identity_7x7': ((7, 7), (7, 7), None),
    'one_pixel_1x3': ((1, 3), (4, 2), None),
    'one_pixel_33x40': ((33, 40), (32, 1), None),
    'mixed_128': ((128, 128), (48, 80), None),
    'scale_factor_20x30': ((20, 30), None, (0.37, 0.61)),
}


@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('name', sorted(TORCH_CASES))
def test_restatement_equals_torch_float64(name, mode):
    in_size, size, scale_factor = TORCH_CASES[name]
    out_size, scales = R.output_size(in_size, size, scale_factor), R.kernel_scales(scale_factor)
    x = torch.from_numpy(R.image(1, 2, in_size))
    if name == 'one_pixel_33x40':
        # torch's CPU kernel is wrong by 0.44 on this shape for a CONTIGUOUS input; its channels_last path is right
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y = F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode, align_corners=False, antialias=True)
    assert tuple(y.shape[2:]) == out_size
    g = torch.from_numpy(R.image(1, 2, out_size, seed=5))
    dx, = torch.autograd.grad(y, x, g)
    err_y = np.abs(y.detach().numpy() - R.forward(x.detach().numpy(), out_size, mode, scales)).max()
    err_dx = np.abs(dx.numpy() - R.transposed(g.numpy(), in_size, mode, scales)).max()
    print(f'{name}/{mode}: value {err_y:.2e}, gradient {err_dx:.2e}')
    assert err_y <= 1e-12 and err_dx <= 1e-12


def test_size_ratio_is_not_the_given_scale():
    """The scale_factor case tells the two readings apart: with the size ratio in place of the given scale the result is off by 0.1 and more."""
    in_size, out_size, scales = R.case('scale_factor_20x30')
    x = R.image(1, 1, in_size)
    assert np.abs(R.forward(x, out_size, 'bilinear', scales) - R.forward(x, out_size, 'bilinear')).max() > 0.1


def test_transposed_is_the_adjoint():
    for name in R.CASES:
        in_size, out_size, scales = R.case(name)
        x, g = R.image(1, 1, in_size), R.image(1, 1, out_size, seed=3)
        a, b = (R.forward(x, out_size, 'bicubic', scales) * g).sum(), (x * R.transposed(g, in_size, 'bicubic', scales)).sum()
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a))


ARGS = [dict(size=(10, 14)), dict(size=9), dict(scale_factor=2), dict(scale_factor=(0.37, 0.61)), dict(scale_factor=(0.37, 0.61), recompute_scale_factor=True),
        dict(scale_factor=1.5, recompute_scale_factor=False), dict(scale_factor=[2.0, 0.5])]


@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('kw', ARGS, ids=[str(i) for i in range(len(ARGS))])
def test_cpu_route_is_the_torch_op_and_the_rules_are_its_rules(kw, mode):
    x = torch.from_numpy(R.image(2, 3, (20, 30))).float()
    want = F.interpolate(x, mode=mode, align_corners=False, antialias=True, **kw)
    assert torch.equal(RZ.interpolate_aa(x, mode=mode, **kw), want)
    # the rules: the output size is torch's, and the restatement with the rules' scales is what torch computes
    out_size, scales = RZ.output_size_and_scales((20, 30), kw.get('size'), kw.get('scale_factor'), kw.get('recompute_scale_factor'))
    assert out_size == tuple(want.shape[2:])
    ref = R.forward(x.double().numpy(), out_size, mode, scales)
    assert np.abs(want.double().numpy() - ref).max() <= 2e-5


def test_rules_refuse_what_torch_refuses():
    for kw in (dict(), dict(size=(4, 4), scale_factor=2.0), dict(size=(4, 4, 4)), dict(scale_factor=(2.0, 2.0, 2.0)), dict(size=(4, 4), recompute_scale_factor=True)):
        with pytest.raises(ValueError):
            RZ.output_size_and_scales((8, 8), kw.get('size'), kw.get('scale_factor'), kw.get('recompute_scale_factor'))
        with pytest.raises((ValueError, RuntimeError, TypeError)):
            F.interpolate(torch.zeros(1, 1, 8, 8), mode='bilinear', antialias=True, **kw)
    with pytest.raises(ValueError, match='mode'):
        RZ.interpolate_aa(torch.zeros(1, 1, 8, 8), size=(4, 4), mode='nearest')


def test_resize_declarations():
    import gnerf_hip
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert int(re.search(r'#define GNERF_ABI_VERSION (\d+)', header).group(1)) == gnerf_hip.ABI_VERSION == 15
    assert int(re.search(r'#define GNERF_RESIZE_MAX_TAPS (\d+)', header).group(1)) == gnerf_hip.RESIZE_MAX_TAPS == 65
    for mode, code in gnerf_hip.RESIZE_MODES.items():
        assert int(re.search(r'#define GNERF_RESIZE_%s (\d+)' % mode.upper(), header).group(1)) == code
    p, i, d, i64p = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('gnerf_resize_aa_forward', 'gnerf_resize_aa_backward'):
        assert gnerf_hip.SIGNATURES[name] == (i, [p, p, i, i, i, i, i, i, i, i64p, i64p, i, d, d, p])
        assert name in gnerf_hip.OPTIONAL_SYMBOLS                   # a library of the same version built before them still loads
        args = re.search(name + r'\s*\((.*?)\)\s*;', header, flags=re.S).group(1)
        assert len(args.split(',')) == len(gnerf_hip.SIGNATURES[name][1]), name
        assert hasattr(gnerf_hip.load(), name)
    assert gnerf_hip.resize_aa_available()
    for name in ('resize_aa_forward', 'resize_aa_backward', 'resize_aa_supported'):
        assert callable(getattr(gnerf_hip, name))
    csrc = os.path.join(ROOT, 'g-nerf_amd', 'csrc')             # build.sh builds the units that compile_unit.sh lists
    assert re.search(r'^for src in \$UNITS;', open(os.path.join(csrc, 'build.sh')).read(), flags=re.M)
    assert re.search(r'^UNITS="[^"]*\bresize\b', open(os.path.join(csrc, 'compile_unit.sh')).read(), flags=re.M)


def test_c_entry_points_refuse_without_a_gpu():
    """Argument checks and the band limits come before any launch, so they answer on a machine without a GPU."""
    import gnerf_hip
    lib = gnerf_hip.load()
    st = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    buf = ctypes.create_string_buffer(64)                            # a non-null pointer that no refused call reads
    ptr = ctypes.addressof(buf)

    def call(fn, in_hw, out_hw, mode=0, n=1, c=1, dtype=0, scales=(0.0, 0.0), x=ptr, y=ptr):
        return fn(x, y, dtype, n, c, in_hw[0], in_hw[1], out_hw[0], out_hw[1], st, st, mode, scales[0], scales[1], None)
    for fn in (lib.gnerf_resize_aa_forward, lib.gnerf_resize_aa_backward):
        assert call(fn, (8, 8), (4, 4), x=None) == -1 and b'null' in lib.gnerf_last_error()
        assert call(fn, (8, 8), (4, 4), dtype=2) == -1 and b'dtype' in lib.gnerf_last_error()
        assert call(fn, (8, 8), (4, 4), mode=2) == -1 and b'mode' in lib.gnerf_last_error()
        assert call(fn, (8, 0), (4, 4)) == -1 and b'empty' in lib.gnerf_last_error()
        assert call(fn, (200, 8), (3, 8)) == gnerf_hip.E_UNSUPPORTED and b'taps' in lib.gnerf_last_error()
        assert call(fn, (8, 3), (8, 200)) == gnerf_hip.E_UNSUPPORTED and b'touch' in lib.gnerf_last_error()
        assert call(fn, (264, 8), (8, 8)) == gnerf_hip.E_UNSUPPORTED                  # scale 33
        assert call(fn, (136, 8), (8, 8), mode=1) == gnerf_hip.E_UNSUPPORTED          # scale 17, bicubic
        assert call(fn, (128, 8), (4, 4), scales=(33.0, 0.0)) == gnerf_hip.E_UNSUPPORTED
        assert call(fn, (1 << 12, 1 << 12), (1 << 11, 1 << 11), n=1 << 4, c=1 << 3) == gnerf_hip.E_UNSUPPORTED and b'2^31' in lib.gnerf_last_error()
    # the Python rule is the library's
    assert not gnerf_hip.resize_aa_supported((1, 1, 200, 8), (3, 8)) and not gnerf_hip.resize_aa_supported((1, 1, 8, 3), (8, 200))
    assert not gnerf_hip.resize_aa_supported((1, 1, 264, 8), (8, 8)) and gnerf_hip.resize_aa_supported((1, 1, 256, 8), (8, 8))
    assert not gnerf_hip.resize_aa_supported((1, 1, 136, 8), (8, 8), 'bicubic') and gnerf_hip.resize_aa_supported((1, 1, 128, 8), (8, 8), 'bicubic')
    assert not gnerf_hip.resize_aa_supported((1, 1, 128, 8), (4, 4), scales=(33.0, None)) and gnerf_hip.resize_aa_supported((1, 1, 8, 8), (256, 256))
    assert not gnerf_hip.resize_aa_supported((1, 1, 8, 8), (272, 272)) and not gnerf_hip.resize_aa_supported((16, 8, 1 << 12, 1 << 12), (2048, 2048))
    # a band is never longer than the axis it reads: 40 -> 1 is 40 taps in either mode, 8 -> 4 at a given scale of 33 is 8
    assert gnerf_hip.resize_aa_supported((1, 1, 33, 40), (32, 1), 'bicubic') and gnerf_hip.resize_aa_supported((1, 1, 8, 8), (4, 4), scales=(33.0, None))
    assert gnerf_hip.resize_aa_supported((4, 3, 512, 512), (64, 64)) and gnerf_hip.resize_aa_supported((4, 32, 64, 64), (128, 128))
    # CPU tensors never reach the library
    with pytest.raises(RuntimeError):
        gnerf_hip.resize_aa_forward(torch.zeros(1, 1, 8, 8), (4, 4))
    with pytest.raises(RuntimeError):
        gnerf_hip.resize_aa_backward(torch.zeros(1, 1, 4, 4), (8, 8))


# ---------------------------------------------------------------------------------------------------------------------
# the op's GPU branch without a GPU: the two library calls are replaced by the restatement and every tensor counts as a GPU tensor


@pytest.fixture
def pretend_gpu(monkeypatch):
    import gnerf_hip
    calls = []

    def fwd(x, out_size, mode='bilinear', scales=(None, None)):
        calls.append(('forward', tuple(x.shape), tuple(out_size), mode, tuple(scales)))
        return torch.from_numpy(R.forward(x.detach().double().numpy(), tuple(out_size), mode, tuple(scales))).to(x.dtype)

    def bwd(dy, in_size, mode='bilinear', scales=(None, None)):
        calls.append(('backward', tuple(dy.shape), tuple(in_size), mode, tuple(scales)))
        return torch.from_numpy(R.transposed(dy.detach().double().numpy(), tuple(in_size), mode, tuple(scales))).to(dy.dtype)

    monkeypatch.setattr(gnerf_hip, 'resize_aa_forward', fwd)
    monkeypatch.setattr(gnerf_hip, 'resize_aa_backward', bwd)
    monkeypatch.setattr(RZ, '_on_gpu', lambda x: True)
    monkeypatch.setattr(RZ, '_warned_fallbacks', set())
    monkeypatch.delenv('GNERF_RESIZE_AA', raising=False)
    return calls


def test_kernel_route_and_its_gradients_to_second_order(pretend_gpu):
    """The Function's backward is the Function again: first and second order gradients are the transposed and the forward operator."""
    in_size, out_size, scales = R.case('scale_factor_20x30')
    x = torch.from_numpy(R.image(1, 2, in_size)).float().requires_grad_(True)
    y = RZ.interpolate_aa(x, scale_factor=(0.37, 0.61), mode='bicubic')
    assert pretend_gpu == [('forward', (1, 2, 20, 30), out_size, 'bicubic', scales)]
    ref = F.interpolate(x.detach(), scale_factor=(0.37, 0.61), mode='bicubic', align_corners=False, antialias=True)
    assert (y - ref).abs().max() <= 1e-5
    g = torch.from_numpy(R.image(1, 2, out_size, seed=2)).float().requires_grad_(True)
    dx, = torch.autograd.grad(y, x, g, create_graph=True)
    assert pretend_gpu[-1] == ('backward', (1, 2, *out_size), in_size, 'bicubic', scales)
    assert np.abs(dx.detach().double().numpy() - R.transposed(g.detach().double().numpy(), in_size, 'bicubic', scales)).max() <= 1e-5
    v = torch.from_numpy(R.image(1, 2, in_size, seed=4)).float()
    dg, = torch.autograd.grad(dx, g, v)                             # d <dx, v> / dg = A v
    assert pretend_gpu[-1][0] == 'forward' and len(pretend_gpu) == 3
    assert np.abs(dg.double().numpy() - R.forward(v.double().numpy(), out_size, 'bicubic', scales)).max() <= 1e-5
    # R1-style: the gradient's square, differentiated again
    x2 = x.detach().clone().requires_grad_(True)
    y2 = RZ.interpolate_aa(x2, size=(7, 9)).square().sum()
    d1, = torch.autograd.grad(y2, x2, create_graph=True)
    d1.square().sum().backward()
    xr = x.detach().double().requires_grad_(True)
    yr = F.interpolate(xr, size=(7, 9), mode='bilinear', align_corners=False, antialias=True).square().sum()
    r1, = torch.autograd.grad(yr, xr, create_graph=True)
    r1.square().sum().backward()
    assert (x2.grad.double() - xr.grad).abs().max() <= 1e-4 * float(xr.grad.abs().max())


def test_env_switch_is_honoured(pretend_gpu, monkeypatch):
    x = torch.from_numpy(R.image(1, 1, (8, 8))).float()
    RZ.interpolate_aa(x, size=(16, 16))
    assert len(pretend_gpu) == 1
    monkeypatch.setenv('GNERF_RESIZE_AA', '0')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        y = RZ.interpolate_aa(x, size=(16, 16))
    assert len(pretend_gpu) == 1 and torch.equal(y, F.interpolate(x, size=(16, 16), mode='bilinear', align_corners=False, antialias=True))
    monkeypatch.setenv('GNERF_RESIZE_AA', '1')
    RZ.interpolate_aa(x, size=(16, 16))
    assert len(pretend_gpu) == 2


def test_fallback_warns_once_per_reason(pretend_gpu):
    big, wide = torch.zeros(1, 1, 200, 8), torch.zeros(1, 1, 8, 3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for _ in range(2):
            assert RZ.interpolate_aa(big, size=(3, 8)).shape == (1, 1, 3, 8)                       # a band over the limit, down
            assert RZ.interpolate_aa(wide, size=(8, 200)).shape == (1, 1, 8, 200)                  # ... and up: the same reason
            assert RZ.interpolate_aa(torch.zeros(1, 1, 8, 8, dtype=torch.float64), size=(4, 4)).dtype == torch.float64
            with pytest.raises((RuntimeError, ValueError, NotImplementedError)):                   # torch's own refusal of a 3-D input
                RZ.interpolate_aa(torch.zeros(1, 8, 8), size=(4,))
    messages = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning) and 'interpolate_aa' in str(w.message)]
    assert len(messages) == 3 and len(set(messages)) == 3, messages
    assert any('band' in m for m in messages) and any('float64' in m for m in messages) and any('4-D' in m for m in messages)
    assert pretend_gpu == []


# ---------------------------------------------------------------------------------------------------------------------
# the callers


class _Spy:
    def __init__(self, monkeypatch):
        self.calls = []
        real = RZ.interpolate_aa

        def spy(x, *args, **kw):
            self.calls.append((tuple(x.shape), args, kw))
            return real(x, *args, **kw)
        monkeypatch.setattr(RZ, 'interpolate_aa', spy)


class _PassThrough(torch.nn.Module):
    def forward(self, x, rgb, ws, noise_mode='none', **kw):
        return x, rgb


@pytest.mark.parametrize('antialias', [True, False])
def test_superresolution_resizes_through_the_op(monkeypatch, antialias):
    import gnerf_generator as GG
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    sr = GG.SuperRes8XDC(32, 512, use_fp16=False, antialias=antialias)
    sr.block0, sr.block1 = _PassThrough(), _PassThrough()            # the 256^2 and 512^2 blocks are not what this test is about
    x, ws = torch.randn(1, 32, 64, 64), torch.randn(1, 14, 512)
    seen = []
    monkeypatch.setattr(sr.block0, 'forward', lambda x, rgb, ws, noise_mode='none', **kw: (seen.append((x, rgb)), (x, rgb))[1])
    rgb, raw = sr(x[:, :3], x, ws)
    (x128, rgb128), = seen
    assert x128.shape == (1, 32, 128, 128) and rgb128.shape == (1, 3, 128, 128) and raw.shape == (1, 3, 64, 64)
    if antialias:
        assert [c[0] for c in spy.calls] == [(1, 32, 64, 64), (1, 3, 64, 64)]
        assert all(c[2].get('size') == (128, 128) and c[2].get('mode', 'bilinear') == 'bilinear' for c in spy.calls)
        assert torch.equal(rgb128, F.interpolate(raw, size=(128, 128), mode='bilinear', align_corners=False, antialias=True))
    else:
        assert spy.calls == []
        assert torch.equal(rgb128, F.interpolate(raw, size=(128, 128), mode='bilinear', align_corners=False, antialias=False))


class _TinyG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(8, 3 * 16 * 16)

    def mapping(self, z, c):
        return z

    def synthesis(self, ws, c, neural_rendering_resolution=None, **kw):
        raw = torch.tanh(self.fc(ws)).view(-1, 3, 16, 16)
        return dict(image=F.interpolate(raw, size=(32, 32), mode='bilinear', align_corners=False), image_raw=raw, image_depth=raw[:, :1] + 2.5)


def test_training_step_resizes_the_real_images_through_the_op(monkeypatch):
    import train_step_mi355x as T
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    batch = dict(z=torch.randn(4, 8), c=torch.zeros(4, 25), loss_image=torch.rand(4, 3, 32, 32) * 2 - 1, factor=torch.tensor([1.0, 0.5, 1.0, 0.0]))
    loss, parts, gen = T.generator_loss(_TinyG(), lambda img, c: img.mean((1, 2, 3)), batch, 16)
    assert [c[0] for c in spy.calls] == [(4, 3, 32, 32)] and spy.calls[0][2].get('size') == (16, 16)
    real_raw = F.interpolate(batch['loss_image'], size=(16, 16), mode='bilinear', align_corners=False, antialias=True)
    want = (real_raw - gen['image_raw'].float()).abs().mean((1, 2, 3)).mean()
    assert torch.equal(parts['l1_raw'], want.detach())
