"""The decoder pack of the fused renderer (gnerf_render_pack_decoder, gnerf_render_forward_packed; csrc/render_shade.inl has the layout).
A pack holds what every workgroup of the pipelined kernels otherwise works out of the decoder before its first ray -- the range
statistics behind the choice of decoder arithmetic and the weights in their LDS layout -- so a packed call must equal the plain call
BIT FOR BIT and choose the same arithmetic: at the smallest shapes that reach each instantiation, through both bindings and both plane
layouts, on either side of every threshold of the choice, after the weights change in place, and in a replayed HIP graph."""

import math

import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.production_path]

RAY_START, RAY_END, BOX_WARP = 2.25, 3.3, 1.0
RES, PLANE = 16, 32                     # one item of 16x16 rays (256: workgroups straddle dealing units) on 32x32 planes
NAMES = ('rgb', 'depth', 'weights_sum')


@pytest.fixture(scope='module')
def dev():
    if not has_gpu():
        pytest.fail('GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)')
    import gnerf_hip
    gnerf_hip.load()
    assert gnerf_hip.decoder_pack_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def base(dev):
    """Planes (NCHW, on the CPU), decoder, camera rays: made once, never modified (the tests scale copies).
    Planes of standard deviation 2 (max |planes| 8.6): loud enough that the scaled cases below -- planes x 20, weights x 5 -- lie beyond
    the error bound that hands a call to fp32 by a fifth or more (decoder_pack_ref.decision restates the bound; the test checks the
    margin), and quiet enough that the unscaled scene is a tenth of the way there."""
    from oracle import render_ref as R
    g = torch.Generator().manual_seed(14)
    planes = 2.0 * torch.randn(1, 3, 32, PLANE, PLANE, generator=g)
    dec = (torch.randn(64, 32, generator=g) / math.sqrt(32), 0.1 * torch.randn(64, generator=g),
           torch.randn(33, 64, generator=g) / math.sqrt(64), 0.1 * torch.randn(33, generator=g))
    c2w = R.lookat_pose(3.14 / 2 + 0.2, 3.14 / 2 - 0.1, 2.7)
    intr = torch.tensor([[4.2647, 0, 0.5], [0, 4.2647, 0.5], [0, 0, 1]])[None]
    o, d = R.make_rays(c2w, intr, RES)
    noise = {n: torch.rand(RES * RES, n, generator=g) for n in (24, 40, 48, 96, 160)}
    return dict(planes=planes, dec=dec, o=o.contiguous(), d=d.contiguous(), noise=noise)


def _planes(base, dev, scale=1.0, interleaved=False):
    import gnerf_hip
    planes = (base['planes'] * scale).to(dev)
    if interleaved:
        nhwc = planes.permute(0, 3, 4, 1, 2).reshape(1, PLANE, PLANE, 96).contiguous()
        return nhwc, gnerf_hip.planes_absmax(nhwc)
    return gnerf_hip.planes_to_nhwc(planes, with_absmax=True)


def _render(base, dev, nhwc, amax, dec, S, F, decoder_pack):
    """decoder_pack=True: the cached pack, which render_forward makes when it sees a decoder the second time -- so the call is made twice
    and the second one, which must have found a pack, is returned."""
    import gnerf_hip
    from gnerf_hip import _native
    if decoder_pack is True:
        _render(base, dev, nhwc, amax, dec, S, F, None)
    out = gnerf_hip.render_forward(nhwc, 1, dec, base['o'].to(dev), base['d'].to(dev), base['noise'][S].to(dev), base['noise'][F].to(dev),
                                   depth_resolution=S, depth_resolution_importance=F, ray_start=RAY_START, ray_end=RAY_END, box_warp=BOX_WARP,
                                   image_width=RES, planes_absmax=amax, decoder_pack=True if decoder_pack is None else decoder_pack)
    if decoder_pack is True:
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, *(v for t in dec for v in (t.data_ptr(), t._version)))
        assert key in _native._decoder_packs, 'the second call with these weights made no pack'
    return out, gnerf_hip.last_mlp_choice(dev)


def _assert_same(a, b, what, finite=True):
    """bit for bit (compared as integers: a NaN weight's NaN outputs must match too)"""
    for name, x, y in zip(NAMES, a, b):
        assert not finite or bool(torch.isfinite(y).all()), (what, name)
        differ = x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)
        assert not bool(differ.any()), f'{what}: {name} differs between the packed and the plain call in {int(differ.sum())} values'


# 48+48: pipe<1>, compile-time counts   96+96: pipe<2>   40+24: the general instantiation   160+160: the generic kernel (reads no pack)
@pytest.mark.parametrize('interleaved', [False, True])
@pytest.mark.parametrize('binding', ['ext', 'ctypes'])
@pytest.mark.parametrize('S,F', [(48, 48), (96, 96), (40, 24), (160, 160)])
def test_packed_call_equals_plain_call_bit_for_bit(dev, base, S, F, binding, interleaved, monkeypatch):
    from gnerf_hip import _native
    assert _native.ext() is not None, 'the default binding is the extension'
    if binding == 'ctypes':
        monkeypatch.setattr(_native, '_ext', False)
    nhwc, amax = _planes(base, dev, interleaved=interleaved)
    dec = tuple(t.to(dev) for t in base['dec'])
    plain, choice_plain = _render(base, dev, nhwc, amax, dec, S, F, False)
    packed, choice_packed = _render(base, dev, nhwc, amax, dec, S, F, True)
    _assert_same(plain, packed, f'{S}+{F} {binding}')
    if S <= 96:
        assert choice_plain == choice_packed == 'f16x3'
    import gnerf_hip
    by_hand, _ = _render(base, dev, nhwc, amax, dec, S, F, gnerf_hip.pack_decoder(dec))        # a pack the caller made
    _assert_same(plain, by_hand, f'{S}+{F} {binding} own pack')


def _h_hard(base):
    """choose_mlp's bound of the base-2 pre-activations at planes scale 1, as (slope, offset): h = slope * scale + offset."""
    w1, b1 = base['dec'][0].double(), base['dec'][1].double()
    l2e = 1.4426950408889634
    return float((w1.abs() * l2e).sum(1).max() * base['planes'].abs().max()), float(b1.abs().max() * l2e + 1.0)


# (planes scale or the bound of the pre-activations to reach, weights scale, NaN weight) -> the arithmetic both calls must choose
RANGE_CASES = {
    'plain': (1.0, 1.0, False, 'f16x3'),
    'direct_softplus_below_limit': ('h=90', 1.0, False, 'f16x3'),       # kSoftplusDirectLimit = 100: the short softplus ...
    'direct_softplus_above_limit': ('h=110', 1.0, False, 'f16x3'),      # ... and the form that is safe for any pre-activation
    'planes_x20': (20.0, 1.0, False, 'f32'),
    'weights_x5': (1.0, 5.0, False, 'f32'),
    'nan_weight': (1.0, 1.0, True, 'f32'),
}


@pytest.mark.parametrize('case', sorted(RANGE_CASES))
def test_same_choice_and_outputs_on_the_range_cases(dev, base, case):
    scale, wscale, nan, want = RANGE_CASES[case]
    if isinstance(scale, str):
        slope, offset = _h_hard(base)
        scale = (float(scale[2:]) - offset) / slope
    import decoder_pack_ref as DR
    nhwc, amax = _planes(base, dev, scale)
    dec = [t * wscale for t in base['dec']]
    if nan:
        dec[2][5, 7] = float('nan')
    # the case lies where its name says, with room for the kernel's float32 evaluation of the same inequalities
    choice, direct, e_o, h_hard = DR.decision(*(t.numpy() for t in dec), float(amax))
    assert choice == want and direct == (case in ('plain', 'direct_softplus_below_limit')), (case, choice, direct, e_o, h_hard)
    assert nan or (abs(e_o / DR.ERR_LIMIT - 1) > 0.1 and abs(h_hard / DR.SOFTPLUS_DIRECT_LIMIT - 1) > 0.05), (case, e_o, h_hard)
    dec = tuple(t.to(dev) for t in dec)
    plain, choice_plain = _render(base, dev, nhwc, amax, dec, 48, 48, False)
    packed, choice_packed = _render(base, dev, nhwc, amax, dec, 48, 48, True)
    assert choice_plain == want and choice_packed == want, (case, choice_plain, choice_packed)
    _assert_same(plain, packed, case, finite=not nan)


def test_cache_misses_follow_the_weights(dev, base):
    nhwc, amax = _planes(base, dev)
    dec = tuple(t.to(dev).clone() for t in base['dec'])
    before, _ = _render(base, dev, nhwc, amax, dec, 48, 48, True)
    dec[0].mul_(1.5)                                            # in place: same address, next version
    after, _ = _render(base, dev, nhwc, amax, dec, 48, 48, True)
    fresh, _ = _render(base, dev, nhwc, amax, dec, 48, 48, False)
    assert not torch.equal(before[0], after[0])
    _assert_same(fresh, after, 'after w1.mul_(1.5)')


def _graph_scene(base, dev):
    import gnerf_hip
    nhwc, amax = _planes(base, dev)
    dec = tuple(t.to(dev).clone() for t in base['dec'])
    inputs = [base[k].to(dev) for k in ('o', 'd')] + [base['noise'][48].to(dev), base['noise'][48].to(dev)]

    def call(decoder_pack=True):
        return gnerf_hip.render_forward(nhwc, 1, dec, *inputs, depth_resolution=48, depth_resolution_importance=48, ray_start=RAY_START, ray_end=RAY_END,
                                        box_warp=BOX_WARP, image_width=RES, planes_absmax=amax, decoder_pack=decoder_pack)
    return dec, call


def _capture(call, **kw):
    """call() captured on a side stream after a warm-up there (workspace; two sights, so that the cache HOLDS a pack for that stream)"""
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(**kw)
        call(**kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    from gnerf_hip import _native
    held = (list(_native._decoder_packs), list(_native._decoder_seen))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call(**kw)
    assert held == (list(_native._decoder_packs), list(_native._decoder_seen)), 'a capture touched the pack cache'
    return graph, out


def _replay(graph, out):
    for t in out:
        t.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    return out


def test_a_captured_default_call_uses_no_cached_pack(dev, base):
    """A capture keeps addresses, the cache may drop any pack: inside a capture the default call is the plain one.  So a replay survives
    the cache's eviction of everything it held at capture time, and follows an in-place update of the weights as the plain call always
    has."""
    import gnerf_hip
    from gnerf_hip import _native
    dec, call = _graph_scene(base, dev)
    call()
    eager = call()                                              # (the second call with these weights: packed)
    packs = dict(_native._decoder_packs)
    graph, out = _capture(call)
    assert any(k[2] == dec[0].data_ptr() and k not in packs for k in _native._decoder_packs)      # the warm-up made the side stream's pack
    _assert_same(eager, _replay(graph, out), 'replay')
    # everything the cache held goes, and its blocks are handed out again and overwritten
    _native._decoder_packs.clear()
    _native._decoder_seen.clear()
    del packs
    junk = [torch.full([int(gnerf_hip.load().gnerf_render_decoder_pack_bytes())], 0xff, dtype=torch.uint8, device=dev) for _ in range(32)]
    torch.cuda.synchronize()
    _assert_same(eager, _replay(graph, out), 'replay after the cache was emptied')
    del junk
    # an in-place update between capture and replay
    dec[0].mul_(1.5)
    fresh = call(decoder_pack=False)
    assert not torch.equal(fresh[0], eager[0])
    _assert_same(fresh, _replay(graph, out), 'replay after w1.mul_(1.5)')


def test_a_captured_call_with_the_callers_pack_keeps_its_weights(dev, base):
    """decoder_pack=<tensor>: the weights are frozen at pack_decoder's call for as long as that pack is passed, in replays too."""
    import gnerf_hip
    dec, call = _graph_scene(base, dev)
    eager = call(decoder_pack=False)
    pack = gnerf_hip.pack_decoder(dec)
    graph, out = _capture(call, decoder_pack=pack)
    _assert_same(eager, _replay(graph, out), 'replay with the caller\'s pack')
    dec[0].mul_(1.5)
    torch.cuda.synchronize()
    _assert_same(eager, _replay(graph, out), 'replay with the caller\'s pack after w1.mul_(1.5)')      # the pack's weights, not the tensors'
    _assert_same(call(decoder_pack=False), call(decoder_pack=gnerf_hip.pack_decoder(dec)), 'a new pack')


@pytest.mark.parametrize('case', ['plain', 'nan_weight', 'inf_bias'])
def test_pack_statistics_match_the_restatement(dev, base, case):
    """The head of the pack against tests/decoder_pack_ref.py, which restates the kernel's pinned operations in its summation order:
    bit for bit."""
    import numpy as np
    import decoder_pack_ref as DR
    import gnerf_hip
    dec = [t.clone() for t in base['dec']]
    if case == 'nan_weight':
        dec[2][5, 7] = float('nan')
    if case == 'inf_bias':
        dec[1][3] = float('inf')
    pack = gnerf_hip.pack_decoder(tuple(t.to(dev) for t in dec))
    assert pack.dtype == torch.uint8 and pack.numel() == DR.PACK_BYTES
    head = pack[:4 * DR.STAT_WORDS].cpu().numpy()
    got, flag = head.view(np.float32), head.view(np.int32)
    want, bad = DR.statistics(*(t.numpy() for t in dec))
    assert int(flag[7]) == int(bad) == (0 if case == 'plain' else 1) and not flag[8:].any()
    for i, name in enumerate(DR.STAT_NAMES):
        assert got[i:i + 1].view(np.int32)[0] == np.float32(want[name]).reshape(1).view(np.int32)[0], (name, got[i], want[name])
    # the f32 image is the padded rows themselves
    img = pack[4 * (DR.STAT_WORDS + DR.IMAGE_FLOATS_F16):].cpu().numpy().view(np.float32)
    if case == 'plain':
        assert np.array_equal(img[:64 * 36].reshape(64, 36)[:, :32], dec[0].numpy()) and not img[:64 * 36].reshape(64, 36)[:, 32:].any()
        assert np.array_equal(img[64 * 36:64 * 36 + 33 * 68].reshape(33, 68)[:, :64], dec[2].numpy())
        assert np.array_equal(img[64 * 36 + 33 * 68:][:64], dec[1].numpy()) and np.array_equal(img[64 * 36 + 33 * 68 + 64:][:33], dec[3].numpy())
