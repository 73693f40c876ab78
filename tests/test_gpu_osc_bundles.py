"""fx_get_osc_bundles / fx_get_osc_bundles_addressed: many tracks' OSC feature messages (ref OSCFeatureAnalysisOutput.h:107) per datagram,
as OSC 1.0 bundles formed on the device in one launch (csrc/fx_osc_bundle.hip).  Bar: bitwise the host encoders fx_osc_encode_bundles*
(held to an independent model and to fx_osc_encode in tests/test_osc_bundles_cpu.py) of fx_get_smoothed -- prefix form and table form,
to host memory and to a device tensor, on a fresh context and after three hops of noise at window 1024 on a spectral-only context (real
values, NaN in the harmonic slots); not one byte written past num_bundles * stride.

Tracks per bundle K in {1, 2, 17, 65, 257, 818}: a bundle inside one wavefront, across two, across the 256-thread workgroup's scan
rounds, and the most a datagram allows; C in {1, K - 1, K, K + 1, 2K + 1}: a short last bundle, a single bundle, a bundle of one.
K follows from max_datagram_bytes and the longest message: 96, 176 and 65 507 bytes give 1, 2 and 818 for 76-byte messages
("/Aud/A<n>", whose elements are 72 and 76 bytes), 1472 gives 17 for 80-byte ones ("/Audio/Trk<n>": 76 and 80 bytes), and
16 + K * (4 + longest) gives the others."""
import ctypes

import numpy as np
import pytest

import osc_address_cases as cases
import signals

pytestmark = pytest.mark.gpu

N = 1024
TAG = 0xE9B1C2D3_40000001
IP = ctypes.POINTER(ctypes.c_int)
SPARE = 4096
# K -> (prefix, max_datagram_bytes) of the prefix form
PREFIX_FORM = {1: ("/Aud/A", 96), 2: ("/Aud/A", 176), 17: ("/Audio/Trk", 1472), 65: ("/Aud/A", 16 + 65 * 80), 257: ("/Aud/A", 16 + 257 * 80), 818: ("/Aud/A", 65507)}
_noise = {}


def _hops(C):
    """three hops of noise per track, every track at its own level (made once for the largest context, shared)"""
    if "x" not in _noise:
        _noise["x"] = signals.loud_noise(2100, 3, N, seed=77) * (0.05 + 0.9 * np.arange(2100, dtype=np.float32)[:, None, None] / 2100)
    return np.ascontiguousarray(_noise["x"][:C], np.float32)


def _counts(K):
    return sorted({C for C in (1, K - 1, K, K + 1, 2 * K + 1) if 1 <= C <= 2100})


def _short_addresses(C):
    """address lengths 1 .. 8, every residue mod 4: messages of 68, 72 and 76 bytes side by side"""
    return [cases.address(1 + c % 8, c) for c in range(C)]


def _to_host(fx, an, addressed, prefix, first, max_bytes, bundles, stride):
    """FX_MEM_HOST into the caller's buffer, SPARE bytes longer than needed and pre-filled with 0xA5"""
    buf = np.full(bundles * stride + SPARE, 0xA5, np.uint8)
    lengths = np.full(bundles, -1, np.int32)
    ptr, lp = buf.ctypes.data_as(ctypes.c_void_p), lengths.ctypes.data_as(IP)
    if addressed:
        fx.capi.check(an._lib.fx_get_osc_bundles_addressed(an._h, TAG, max_bytes, ptr, stride, lp, fx.capi.MEM_HOST))
    else:
        fx.capi.check(an._lib.fx_get_osc_bundles(an._h, prefix.encode(), first, TAG, max_bytes, ptr, stride, lp, fx.capi.MEM_HOST))
    launches = an.last_launches()
    assert (buf[bundles * stride:] == 0xA5).all(), "bytes past num_bundles * stride were written (host)"
    return buf[:bundles * stride].reshape(bundles, stride), lengths, launches


def _to_device(fx, an, addressed, prefix, first, max_bytes, bundles, stride):
    """FX_MEM_DEVICE into a torch uint8 tensor, SPARE bytes longer than needed and pre-filled with 0xA5"""
    import torch
    buf = torch.full((bundles * stride + SPARE,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lengths = np.full(bundles, -1, np.int32)
    ptr, lp = ctypes.c_void_p(buf.data_ptr()), lengths.ctypes.data_as(IP)
    if addressed:
        fx.capi.check(an._lib.fx_get_osc_bundles_addressed(an._h, TAG, max_bytes, ptr, stride, lp, fx.capi.MEM_DEVICE))
    else:
        fx.capi.check(an._lib.fx_get_osc_bundles(an._h, prefix.encode(), first, TAG, max_bytes, ptr, stride, lp, fx.capi.MEM_DEVICE))
    an.sync()
    got = buf.cpu().numpy()
    assert (got[bundles * stride:] == 0xA5).all(), "bytes past num_bundles * stride were written (device)"
    return got[:bundles * stride].reshape(bundles, stride), lengths


def _check(fx, an, K, addresses=None, prefix=None, first=0, max_bytes=None):
    """both memory kinds of one form against the host encoder of fx_get_smoothed; the launch record"""
    capi = fx.capi
    C = an.num_channels
    latest = an.get_features()
    if addresses is not None:
        longest = an.osc_address_stride()
        want, want_n = capi.osc_encode_bundles_addressed(addresses, latest, TAG, max_bytes)
    else:
        longest = capi.osc_stride(prefix, first, C)
        want, want_n = capi.osc_encode_bundles(prefix, first, latest, TAG, max_bytes)
    planned, bundles, stride = capi.osc_bundle_plan(longest, C, max_bytes)
    assert planned == min(K, C) and want.shape == (bundles, stride)
    got, n, launches = _to_host(fx, an, addresses is not None, prefix, first, max_bytes, bundles, stride)
    assert [r["kind"] for r in launches] == ["osc_bundle"], launches            # exactly one launch, of kind 13
    assert np.array_equal(n, want_n)
    assert np.array_equal(got, want), ("host", K, C, np.argwhere(got != want)[:4])
    got, n = _to_device(fx, an, addresses is not None, prefix, first, max_bytes, bundles, stride)
    assert np.array_equal(n, want_n)
    assert np.array_equal(got, want), ("device", K, C, np.argwhere(got != want)[:4])
    return latest, want, want_n


def _every_form(fx, an, K):
    C = an.num_channels
    prefix, max_bytes = PREFIX_FORM[K]
    latest, _, _ = _check(fx, an, K, prefix=prefix, max_bytes=max_bytes)
    short = _short_addresses(C)
    an.set_osc_addresses(short)
    longest = an.osc_address_stride()
    _check(fx, an, K, addresses=short, max_bytes=65507 if K == 818 else 16 + K * (4 + longest))
    if K in (2, 17, 65, 257):                   # addresses of 1 .. 124 bytes: messages of 68 .. 192 bytes in one bundle
        long = cases.addresses(C, offset=K)
        an.set_osc_addresses(long)
        _check(fx, an, K, addresses=long, max_bytes=16 + K * (4 + an.osc_address_stride()))
    an.set_osc_addresses(None)
    return latest


@pytest.mark.parametrize("K", [1, 2, 17, 65, 257, 818])
def test_device_bundles_equal_the_host_encoder_bitwise(gpu_fx, K):
    fx = gpu_fx
    for C in _counts(K):
        an = fx.BatchAnalyser(C, N, analysers="spectral")
        try:
            fresh = _every_form(fx, an, K)                          # `latest` as fx_create leaves it
            an.push_hops(_hops(C))
            latest = _every_form(fx, an, K)
            assert not np.array_equal(latest, fresh, equal_nan=True)
            assert np.isnan(latest[:, fx.F0]).all()                 # a spectral-only context: getValue's 0/0 in the harmonic slots
        finally:
            an.close()


def test_the_largest_context_and_the_time_tag(gpu_fx):
    fx = gpu_fx
    C = 2100
    an = fx.BatchAnalyser(C, N, analysers="spectral")
    try:
        an.push_hops(_hops(C))
        latest = an.get_features()
        # first_channel 9 999 000: "/Audio/A9999999" -> "/Audio/A10000000" at track 1000, 80 -> 84 bytes inside a bundle
        for max_bytes in (1472, 65507):
            _check(fx, an, fx.capi.osc_bundle_plan(84, C, max_bytes)[0], prefix="/Audio/A", first=9999000, max_bytes=max_bytes)
        # the binding's own call: defaults, "immediately"; and another time tag and datagram size on the next call, nothing to invalidate
        d, n = an.osc_bundles()
        want, want_n = fx.capi.osc_encode_bundles("/Audio/A", 0, latest, 1, 1472)
        assert np.array_equal(d, want) and np.array_equal(n, want_n)
        dev, n = an.osc_bundles(timetag=fx.capi.osc_timetag(1792281600.25), max_datagram_bytes=9000, device=True)
        an.sync()
        want, want_n = fx.capi.osc_encode_bundles("/Audio/A", 0, latest, fx.capi.osc_timetag(1792281600.25), 9000)
        assert np.array_equal(dev.cpu().numpy(), want) and np.array_equal(n, want_n)
    finally:
        an.close()


def test_the_datagram_call_is_untouched(gpu_fx):
    """fx_get_osc_datagrams before and after a bundle call on the same context: the same bytes, the same launch record"""
    fx = gpu_fx
    C = 257
    an = fx.BatchAnalyser(C, N, analysers="spectral")
    try:
        an.push_hops(_hops(C))
        before, before_n = an.osc_datagrams("/Audio/A", 990)
        record = an.last_launches()
        assert [r["kind"] for r in record] == ["osc"]
        an.osc_bundles("/Audio/A", 990, timetag=TAG)
        assert [r["kind"] for r in an.last_launches()] == ["osc_bundle"]
        after, after_n = an.osc_datagrams("/Audio/A", 990)
        assert np.array_equal(before, after) and np.array_equal(before_n, after_n)
        assert an.last_launches() == record
        want, want_n = fx.capi.osc_encode_batch("/Audio/A", 990, an.get_features())
        assert np.array_equal(after, want) and np.array_equal(after_n, want_n)
    finally:
        an.close()


def test_refusals_leave_the_buffer_untouched(gpu_fx):
    import torch
    fx = gpu_fx
    capi = fx.capi
    C = 40
    an = fx.BatchAnalyser(C, N, analysers="spectral")
    try:
        L, h = an._lib, an._h
        K, bundles, stride = capi.osc_bundle_plan(76, C, 1472)
        host = np.full(bundles * stride + SPARE, 0xA5, np.uint8)
        dev = torch.full((bundles * stride + SPARE,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        hp, dp = host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dev.data_ptr())
        bad = capi.FX_ERR_INVALID_ARGUMENT
        # no table for the addressed form
        assert L.fx_get_osc_bundles_addressed(h, TAG, 1472, hp, stride, None, capi.MEM_HOST) == bad
        assert L.fx_get_osc_bundles_addressed(h, TAG, 1472, dp, stride, None, capi.MEM_DEVICE) == bad
        # a misaligned device pointer
        assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, ctypes.c_void_p(dev.data_ptr() + 2), stride, None, capi.MEM_DEVICE) == bad
        for kind, ptr in ((capi.MEM_HOST, hp), (capi.MEM_DEVICE, dp)):
            assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, ptr, stride - 4, None, kind) == bad      # stride too small
            assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, ptr, stride + 2, None, kind) == bad      # no multiple of 4
            assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 95, ptr, stride, None, kind) == bad            # holds no message
            assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 65508, ptr, 65536, None, kind) == bad
            assert L.fx_get_osc_bundles(h, b"/Audio/A", -1, TAG, 1472, ptr, stride, None, kind) == bad
            assert L.fx_get_osc_bundles(h, b"/" + b"x" * 65, 0, TAG, 1472, ptr, stride, None, kind) == bad
        assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, hp, stride, None, 7) == bad
        assert L.fx_get_osc_bundles(h, None, 0, TAG, 1472, hp, stride, None, capi.MEM_HOST) == bad
        assert L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, None, stride, None, capi.MEM_HOST) == bad
        an.sync()
        assert (host == 0xA5).all() and bool((dev == 0xA5).all())
        # and the same arguments made right are taken (lengths NULL)
        capi.check(L.fx_get_osc_bundles(h, b"/Audio/A", 0, TAG, 1472, hp, stride, None, capi.MEM_HOST))
        want, _ = capi.osc_encode_bundles("/Audio/A", 0, an.get_features(), TAG, 1472)
        assert np.array_equal(host[:bundles * stride].reshape(bundles, stride), want) and (host[bundles * stride:] == 0xA5).all()
    finally:
        an.close()


def test_analysis_to_bundles_to_sender_to_receiver(gpu_fx):
    import time
    fx = gpu_fx
    capi = fx.capi
    C = 1024
    an = fx.BatchAnalyser(C, N, analysers="spectral")
    rx = capi.OscReceiver(prefix="/Audio/A", keep_channels=C, bundles=True)
    tx = capi.OscSender("127.0.0.1:%d" % rx.port, threads=2)
    try:
        an.push_hops(_hops(C))
        tag = capi.osc_timetag(1792281600.5)
        d, n = an.osc_bundles("/Audio/A", 0, timetag=tag)
        latest = an.get_features()
        tx.update(d, n)
        assert tx.send() == d.shape[0] == capi.osc_bundle_plan(80, C, 1472)[1]
        deadline = time.monotonic() + 5.0
        while rx.bundle_stats()["elements"] < C and time.monotonic() < deadline:
            time.sleep(0.002)
        assert rx.bundle_stats() == {"bundles": d.shape[0], "elements": C, "last_timetag": tag}
        assert rx.stats()["malformed"] == 0 and rx.stats()["datagrams"] == d.shape[0]
        for c in range(C):
            assert rx.last(c) == fx.osc_encode("/Audio/A%d" % c, latest[c]), c
    finally:
        tx.close()
        rx.close()
        an.close()
