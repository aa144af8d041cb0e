"""The decoder pack's host side without a GPU: render_forward's bounded cache of packs (keying, the stream rule, eviction, what a graph
capture may and may not do) with the launch stubbed out, the numpy restatement of the pack's statistics (tests/decoder_pack_ref.py,
which the GPU test holds the kernel to) against float64, and the three exports' place in the header and the ctypes table."""

import os
import re

import numpy as np
import pytest
import torch

import decoder_pack_ref as DR
from conftest import ROOT

import gnerf_hip
from gnerf_hip import _native, render


def _decoder(seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(64, 32, generator=g), torch.randn(64, generator=g), torch.randn(33, 64, generator=g), torch.randn(33, generator=g))


@pytest.fixture
def stub(monkeypatch):
    """_decoder_pack with everything native replaced: packs are numbered objects, the stream and the capture state are the test's."""
    state = dict(made=[], stream=1, capturing=False, available=True)

    def pack_decoder(decoder):
        state['made'].append(tuple(t.clone() for t in decoder))
        return ('pack', len(state['made']))
    monkeypatch.setattr(render, 'pack_decoder', pack_decoder)
    monkeypatch.setattr(render, '_stream', lambda t: state['stream'])
    monkeypatch.setattr(render, 'decoder_pack_available', lambda: state['available'])
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: state['capturing'])
    monkeypatch.setattr(_native, '_decoder_packs', {})
    monkeypatch.setattr(_native, '_decoder_seen', {})
    return state


def _packed(dec):
    """the pack of a decoder the cache has seen before: first sight makes none"""
    render._decoder_pack(dec)
    return render._decoder_pack(dec)


def test_a_pack_is_made_at_second_sight(stub):
    dec = _decoder()
    assert render._decoder_pack(dec) is None and not stub['made'] and not _native._decoder_packs and len(_native._decoder_seen) == 1
    assert render._decoder_pack(dec) == ('pack', 1) and len(_native._decoder_packs) == 1 and not _native._decoder_seen
    for _ in range(5):                                                  # weights that change before every call never make one
        dec[0].mul_(1.01)
        assert render._decoder_pack(dec) is None
    assert len(stub['made']) == 1


def test_cache_hits_on_the_same_tensors_and_misses_on_a_new_version(stub):
    dec = _decoder()
    first = _packed(dec)
    assert first == ('pack', 1) and render._decoder_pack(dec) is first and len(stub['made']) == 1
    assert render._decoder_pack(tuple(dec)) is first                    # the key is the tensors, not the tuple
    dec[0].mul_(1.5)                                                    # an optimizer step: same address, next version
    second = _packed(dec)
    assert second == ('pack', 2) and torch.equal(stub['made'][1][0], dec[0])
    dec[3].add_(1.0)                                                    # ... of any of the four
    assert _packed(dec) == ('pack', 3)
    other = _decoder(1)
    assert _packed(other) == ('pack', 4) and render._decoder_pack(dec) == ('pack', 3)


def test_cache_keeps_the_tensors_of_its_entries_alive(stub):
    """An entry is found by address and version: the address must not come back under other values while the entry lives."""
    dec = _decoder()
    render._decoder_pack(dec)
    (held,) = _native._decoder_seen.values()
    assert all(a is b for a, b in zip(held, dec))
    render._decoder_pack(dec)
    (entry,) = _native._decoder_packs.values()
    assert all(a is b for a, b in zip(entry[1], dec))


def test_cache_is_bounded_and_evicts_the_least_recently_used(stub):
    decs = [_decoder(i) for i in range(render.DECODER_PACK_CACHE)]
    for d in decs:
        _packed(d)
    assert len(_native._decoder_packs) == render.DECODER_PACK_CACHE == 8
    made = len(stub['made'])
    assert render._decoder_pack(decs[0]) == ('pack', 1) and len(stub['made']) == made              # a hit: decs[0] is now the most recently used
    assert _packed(_decoder(100)) == ('pack', made + 1) and len(_native._decoder_packs) == 8
    assert render._decoder_pack(decs[0]) == ('pack', 1)                                             # still there ...
    assert render._decoder_pack(decs[1]) is None and render._decoder_pack(decs[1]) == ('pack', made + 2)        # ... decs[1] went: two sights again


def test_first_sights_take_no_packs_place(stub):
    """A long-lived decoder keeps its pack through any number of decoders that are seen once each (weights that change before every call)."""
    stay = _decoder()
    assert _packed(stay) == ('pack', 1)
    for i in range(3 * render.DECODER_PACK_CACHE):
        assert render._decoder_pack(_decoder(1 + i)) is None
    assert len(_native._decoder_seen) == render.DECODER_PACK_CACHE and len(_native._decoder_packs) == 1
    assert render._decoder_pack(stay) == ('pack', 1) and len(stub['made']) == 1


def test_streams_hold_a_pack_each(stub):
    dec = _decoder()
    assert _packed(dec) == ('pack', 1)
    stub['stream'] = 2
    assert render._decoder_pack(dec) is None and _packed(dec) == ('pack', 2)                       # the stream is part of the key
    for _ in range(3):                                                                              # alternating streams remake nothing
        stub['stream'] = 1
        assert render._decoder_pack(dec) == ('pack', 1)
        stub['stream'] = 2
        assert render._decoder_pack(dec) == ('pack', 2)
    assert len(stub['made']) == 2 and len(_native._decoder_packs) == 2


def test_a_capture_gets_no_cached_pack(stub):
    dec = _decoder()
    stub['capturing'] = True
    assert render._decoder_pack(dec) is None and not stub['made'] and not _native._decoder_packs and not _native._decoder_seen
    stub['capturing'] = False
    assert _packed(dec) == ('pack', 1)
    stub['capturing'] = True                                             # ... also where the cache holds one: a captured launch keeps addresses,
    assert render._decoder_pack(dec) is None and len(stub['made']) == 1  # the cache may drop any pack before a replay
    stub['capturing'] = False
    assert render._decoder_pack(dec) == ('pack', 1)


def test_what_goes_without_a_pack(stub):
    dec = _decoder()
    assert render._decoder_pack((dec[0].double(), *dec[1:])) is None     # converted copies are new tensors on every call
    assert render._decoder_pack((dec[0].t().contiguous().t(), *dec[1:])) is None
    with torch.inference_mode():
        inf = _decoder(2)
    assert render._decoder_pack(inf) is None                             # inference tensors track no version
    stub['available'] = False                                            # a library built before the exports
    assert render._decoder_pack(dec) is None and not stub['made']


def test_statistics_restatement_against_float64():
    """Each statistic is a maximum over rows of an n-term float32 sum of non-negative terms: within n 2^-24 (relative) of the float64 value
    (every term and every partial sum rounded once; the maxima are exact in any order)."""
    w1, b1, w2, b2 = (t.numpy() for t in _decoder(3))
    got, bad = DR.statistics(w1, b1, w2, b2)
    assert not bad
    l2e = 1.4426950408889634
    a1, a2 = np.abs(w1.astype(np.float64)) * l2e, np.abs(w2.astype(np.float64))
    want = dict(l1=a1.sum(1).max(), sq1=(a1 * a1).sum(1).max(), mx1=a1.max(), sq2=(a2 * a2).sum(1).max(), mx2=a2.max(),
                mb1=np.abs(b1.astype(np.float64)).max() * l2e, mb2=np.abs(b2.astype(np.float64)).max() * l2e)
    terms = dict(l1=32, sq1=32, mx1=1, sq2=64, mx2=1, mb1=1, mb2=1)
    for name in DR.STAT_NAMES:
        assert got[name].dtype == np.float32
        assert abs(float(got[name]) - want[name]) <= (terms[name] + 2) * 2.0 ** -24 * want[name], name
    w2n = w2.copy()
    w2n[5, 7] = np.nan
    got, bad = DR.statistics(w1, b1, w2n, b2)
    assert bad and np.isfinite(got['sq2']) and np.isfinite(got['mx2'])   # fmaxf drops the NaN row: the flag carries it
    assert DR.statistics(w1, np.where(np.arange(64) == 3, np.inf, b1).astype(np.float32), w2, b2)[1]


def test_exports_are_declared_and_optional():
    header = open(os.path.join(ROOT, 'include', 'gnerf_hip.h')).read()
    assert re.search(r'#define\s+GNERF_ABI_VERSION\s+15\b', header) and gnerf_hip.ABI_VERSION == 15
    for name, pattern in (('gnerf_render_decoder_pack_bytes', r'\bsize_t\s+gnerf_render_decoder_pack_bytes\s*\(\s*void\s*\)\s*;'),
                          ('gnerf_render_pack_decoder', r'\bint\s+gnerf_render_pack_decoder\s*\(([^)]*)\)\s*;'),
                          ('gnerf_render_forward_packed', r'\bint\s+gnerf_render_forward_packed\s*\(([^)]*)\)\s*;')):
        m = re.search(pattern, header)
        assert m, f'{name} is not declared'
        assert name in gnerf_hip.SIGNATURES and name in gnerf_hip.OPTIONAL_SYMBOLS          # a library of the same version built before them still loads
        if m.groups():
            assert len(m.group(1).split(',')) == len(gnerf_hip.SIGNATURES[name][1])
    lib = gnerf_hip.load()
    assert gnerf_hip.decoder_pack_available()
    assert lib.gnerf_render_decoder_pack_bytes() == DR.PACK_BYTES and DR.PACK_BYTES % 16 == 0
    assert lib.gnerf_render_forward_packed.argtypes == gnerf_hip.SIGNATURES['gnerf_render_forward_packed'][1]
