"""fx_get_osc_datagrams_addressed: every track's OSC feature message with the track's OWN address (ref AnalyserTrackController.h:17:
each track is built with its bundle address; OSCFeatureAnalysisOutput.h:107 sends it), written on the device from an address table
(csrc/fx_osc_table.hip).  Bar: bitwise fx_osc_encode_addressed (the host twin, itself held to fx_osc_encode and the oracle in
tests/test_osc_addresses_cpu.py) of fx_get_smoothed -- to host and to a device tensor, at the smallest stride and 12 bytes more,
before any frame and after three hops of noise; NaN slots from a spectral-only context.  Window 256; C crosses wavefront and workgroup boundaries with word
counts that do not divide 256; neighbouring tracks differ in address length (1 .. 124 bytes, every residue mod 4)."""
import ctypes

import numpy as np
import pytest

import osc_address_cases as cases
import signals

pytestmark = pytest.mark.gpu

N = 256
IP = ctypes.POINTER(ctypes.c_int)


def _device_datagrams(fx, an, stride):
    """the FX_MEM_DEVICE form into a torch tensor pre-filled with 0xEE: asynchronous on the context's stream"""
    import torch
    C = an.num_channels
    out = torch.full((C, stride), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lengths = np.full(C, -1, np.int32)
    fx.capi.check(an._lib.fx_get_osc_datagrams_addressed(an._h, ctypes.c_void_p(out.data_ptr()), stride, lengths.ctypes.data_as(IP), fx.capi.MEM_DEVICE))
    an.sync()
    return out.cpu().numpy(), lengths


def _check_every_form(fx, an, addr):
    latest = an.get_features()
    smallest = max(cases.message_bytes(a) for a in addr)
    assert an.osc_address_stride() == smallest
    for stride in (smallest, smallest + 12):
        want_d, want_n = fx.capi.osc_encode_addressed(addr, latest, stride=stride)
        assert [int(x) for x in want_n] == [cases.message_bytes(a) for a in addr]
        d, n = an.osc_datagrams(addressed=True, stride=stride)
        assert d.shape == (len(addr), stride) and np.array_equal(n, want_n)
        assert np.array_equal(d, want_d), ("host", stride, np.argwhere(d != want_d)[:4])
        dd, dn = _device_datagrams(fx, an, stride)
        assert np.array_equal(dn, want_n) and np.array_equal(dd, want_d), ("device", stride, np.argwhere(dd != want_d)[:4])
        for c in range(len(addr)):
            assert not d[c, n[c]:].any(), c                       # (implied by the equality: the slots' remainders are zeros)
    d, n = an.osc_datagrams(addressed=True)                       # stride None: the table's own
    assert d.shape[1] == smallest
    assert an.last_launches()[0]["kind"] == "osc_table" and len(an.last_launches()) == 1
    return latest, d, n


@pytest.mark.parametrize("C", [1, 3, 64, 65, 257])
def test_device_datagrams_equal_the_host_twin_bitwise(gpu_fx, C):
    fx = gpu_fx
    an = fx.BatchAnalyser(C, N)
    try:
        addr = cases.addresses(C)
        # without a table the addressed call is refused
        assert an.osc_address_stride() == -1
        with pytest.raises(fx.FxError) as e:
            an.osc_datagrams(addressed=True, stride=192)
        assert e.value.code == fx.capi.FX_ERR_INVALID_ARGUMENT
        an.set_osc_addresses(addr)
        # before any frame: whatever the context's latest vectors hold then (a new context's are zeros) is what the messages carry
        latest0, _, _ = _check_every_form(fx, an, addr)
        hops = signals.loud_noise(C, 3, N, seed=40 + C) * (0.05 + 0.9 * np.arange(C, dtype=np.float32)[:, None, None] / max(C, 2))
        an.push_hops(hops.astype(np.float32))
        latest, d, n = _check_every_form(fx, an, addr)
        assert not np.array_equal(latest, latest0, equal_nan=True)
        if C > 1:
            assert len({latest[c].tobytes() for c in range(C)}) == C               # per-track distinct values
        for c in (0, C // 2, C - 1):
            assert bytes(d[c, :n[c]]) == fx.osc_encode(addr[c], latest[c])
        # the prefix form on the same context is untouched
        pd, pn = an.osc_datagrams("/Audio/A", 990)
        want_d, want_n = fx.capi.osc_encode_batch("/Audio/A", 990, latest)
        assert np.array_equal(pd, want_d) and np.array_equal(pn, want_n)
        assert an.last_launches()[0]["kind"] == "osc"
    finally:
        an.close()


def test_nan_slots_travel_unchanged(gpu_fx):
    """A spectral-only context leaves the harmonic slots at getValue's 0/0 = NaN (RealTimeAnalyser.h:84-88): the NaN's bits reach the
    messages as they are, and the loud noise's flatness = inf with them."""
    fx = gpu_fx
    C = 5
    an = fx.BatchAnalyser(C, N, analysers="spectral")
    try:
        addr = cases.addresses(C, offset=9)
        an.set_osc_addresses(addr)
        an.push_hops(signals.loud_noise(C, 3, N, seed=3))
        latest, _, _ = _check_every_form(fx, an, addr)
        assert np.isnan(latest[:, fx.F0]).all()
    finally:
        an.close()


def test_table_is_a_setting_and_is_replaced_whole(gpu_fx):
    fx = gpu_fx
    C = 65
    an = fx.BatchAnalyser(C, N)
    try:
        addr = cases.addresses(C)
        an.set_osc_addresses(addr)
        an.push_hops(signals.loud_noise(C, 3, N, seed=7))
        # fx_reset_channels and fx_reset_state keep the table (the values change, the addresses do not)
        an.reset_channels([0, 17, 64])
        _check_every_form(fx, an, addr)
        an.reset_state()
        assert an.osc_address_stride() == 192
        _check_every_form(fx, an, addr)
        an.push_hops(signals.loud_noise(C, 2, N, seed=8))
        # a bad entry fails the whole call, names the track and changes nothing
        for bad, track in (("", 0), ("Audio/A", 1), ("/Audio A", 33), ("/Audio/\x7f", 63), ("/" + "x" * 124, 64)):
            broken = list(addr)
            broken[track] = bad
            with pytest.raises(fx.FxError, match="track %d:" % track) as e:
                an.set_osc_addresses([a.encode("latin-1") for a in broken])
            assert e.value.code == fx.capi.FX_ERR_INVALID_ARGUMENT
            assert an.osc_address_stride() == 192
        _check_every_form(fx, an, addr)
        # shorter addresses in place of longer ones: no byte of the old table is left in a row or a slot
        short = ["/%d" % (c % 7) if c % 3 else "/Audio/Features" for c in range(C)]
        an.set_osc_addresses(short)
        assert an.osc_address_stride() == 80
        latest, d, n = _check_every_form(fx, an, short)
        assert bytes(d[1, :n[1]]) == fx.osc_encode("/1", latest[1]) and n[1] == 68
        # at the old, wider stride too
        wide_d, wide_n = an.osc_datagrams(addressed=True, stride=192)
        want_d, want_n = fx.capi.osc_encode_addressed(short, latest, stride=192)
        assert np.array_equal(wide_d, want_d) and np.array_equal(wide_n, want_n)
        # strides the table does not allow, and a misaligned device buffer
        for stride in (76, 82, 0):
            with pytest.raises(fx.FxError):
                an.osc_datagrams(addressed=True, stride=stride)
        import torch
        buf = torch.zeros(C * 80 + 4, dtype=torch.uint8, device="cuda:0")
        assert an._lib.fx_get_osc_datagrams_addressed(an._h, ctypes.c_void_p(buf.data_ptr() + 1), 80, None, fx.capi.MEM_DEVICE) == fx.capi.FX_ERR_INVALID_ARGUMENT
        assert an._lib.fx_get_osc_datagrams_addressed(an._h, ctypes.c_void_p(buf.data_ptr()), 80, None, 7) == fx.capi.FX_ERR_INVALID_ARGUMENT
        # NULL drops the table: the addressed call is refused again, the prefix form still works
        an.set_osc_addresses(None)
        assert an.osc_address_stride() == -1
        assert an._lib.fx_get_osc_datagrams_addressed(an._h, ctypes.c_void_p(buf.data_ptr()), 80, None, fx.capi.MEM_DEVICE) == fx.capi.FX_ERR_INVALID_ARGUMENT
        pd, pn = an.osc_datagrams("/Audio/A", 0)
        assert np.array_equal(pd, fx.capi.osc_encode_batch("/Audio/A", 0, latest)[0])
        an.set_osc_addresses(addr)                                   # and a table can be set again
        _check_every_form(fx, an, addr)
    finally:
        an.close()
