"""OSC bundles on the host (include/fx.h: fx_osc_bundle_plan, fx_osc_timetag, fx_osc_encode_bundles, fx_osc_encode_bundles_addressed, the
receiver's FX_OSC_RECEIVER_BUNDLES): many tracks' messages (ref OSCFeatureAnalysisOutput.h:107) per datagram.  Bar: byte identity with
tests/osc_bundle_model.py, an independent builder and parser of the OSC 1.0 bundle layout that shares nothing with the binding, and
with fx_osc_encode for every element; exact counts over real loopback sockets.  No GPU."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import osc_bundle_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 0xE9B1C2D3_40000001           # an arbitrary time tag with every byte different


def _vectors(n, seed=0):
    """[n][12] float32 with what must travel unchanged: NaN with a payload, +-inf, -0.0, denormals"""
    v = np.random.default_rng(seed).standard_normal((n, 12)).astype(np.float32)
    bits = v.view(np.uint32)
    bits[0, 5] = 0x7F800000                     # +inf
    bits[n // 2, 2] = 0x7FC12345                # NaN, payload kept
    bits[n // 2, 9] = 0xFFA00001                # a signalling NaN's bits
    bits[-1, 8] = 0xFF800000                    # -inf
    bits[-1, 0] = 0x80000000                    # -0.0
    bits[n // 3, 1] = 0x00000001                # the smallest denormal
    bits[n // 3, 11] = 0x807FFFFF               # the largest negative denormal
    return v


def _counts(K):
    return sorted({n for n in (1, K - 1, K, K + 1, 2 * K + 1) if n >= 1})


def _check_against_model(fx, out, lengths, addresses, v, max_bytes):
    """out [B][stride] and lengths [B] against the model's datagrams of these tracks; returns K"""
    bits = v.view(np.uint32)
    messages = [model.message(a, bits[c]) for c, a in enumerate(addresses)]
    want, K, stride = model.bundles(messages, TAG, max_bytes)
    assert out.shape == (len(want), stride), (out.shape, len(want), stride)
    assert [int(x) for x in lengths] == [len(d) for d in want]
    for b, d in enumerate(want):
        assert len(d) <= max_bytes
        assert bytes(out[b, :lengths[b]]) == d, (b, K)
        assert not out[b, lengths[b]:].any(), ("slot remainder", b)
        tag, elements = model.parse(out[b, :lengths[b]])
        assert tag == TAG and len(elements) == min(K, len(addresses) - b * K)
        for e, element in enumerate(elements):                      # every element is the track's own message, as fx_osc_encode makes it
            c = b * K + e
            name = addresses[c] if isinstance(addresses[c], str) else addresses[c].decode("latin-1")
            assert element == fx.osc_encode(name, v[c]), c
    return K


def test_plan_at_its_edges(fx):
    capi = fx.capi
    for longest in (76, 80, 192):
        assert capi.osc_bundle_plan(longest, 5, 16 + 4 + longest) == (1, 5, 20 + longest) == model.plan(longest, 5, 20 + longest)
        with pytest.raises(fx.FxError) as e:
            capi.osc_bundle_plan(longest, 5, 16 + 4 + longest - 1)
        assert e.value.code == capi.FX_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            model.plan(longest, 5, 16 + 4 + longest - 1)
    assert capi.osc_bundle_plan(80, 65536, 1472) == (17, 3856, 16 + 17 * 84) == model.plan(80, 65536, 1472)
    assert capi.osc_bundle_plan(76, 65536, 1472) == (18, 3641, 16 + 18 * 80) == model.plan(76, 65536, 1472)
    assert capi.osc_bundle_plan(76, 65536, 65507) == (818, 81, 16 + 818 * 80) == model.plan(76, 65536, 65507)
    assert capi.osc_bundle_plan(192, 65536, 65507) == (334, 197, 16 + 334 * 196) == model.plan(192, 65536, 65507)
    # fewer tracks than a datagram holds: one bundle of them all
    assert capi.osc_bundle_plan(76, 5, 1472) == (5, 1, 16 + 5 * 80) == model.plan(76, 5, 1472)
    assert capi.osc_bundle_plan(76, 1, 65507) == (1, 1, 96)
    # the cap of FX_OSC_BUNDLE_MAX_ELEMENTS (a 4-byte "message" only to reach it: 65491 / 8 = 8186 would fit)
    assert capi.OSC_BUNDLE_MAX_ELEMENTS == 1024
    assert capi.osc_bundle_plan(4, 5000, 65507) == (1024, 5, 16 + 1024 * 8) == model.plan(4, 5000, 65507)
    for bad in ((76, 0, 1472), (76, -3, 1472), (76, 10, 65508), (76, 10, 0), (76, 10, -1)):
        with pytest.raises(fx.FxError) as e:
            capi.osc_bundle_plan(*bad)
        assert e.value.code == capi.FX_ERR_INVALID_ARGUMENT
    # any output pointer may be NULL
    assert fx.load_library().fx_osc_bundle_plan(76, 10, 1472, None, None, None) == capi.FX_OK


def test_timetag(fx):
    capi = fx.capi
    assert capi.OSC_TIMETAG_IMMEDIATE == 1 == model.IMMEDIATE
    assert capi.osc_timetag(0.0) == 2208988800 << 32 == model.timetag(0.0)
    assert capi.osc_timetag(0.5) == (2208988800 << 32) | 0x80000000 == model.timetag(0.5)
    t2026 = 1792281600.25                                              # 2026-10-18 00:00:00.25 UTC
    assert capi.osc_timetag(t2026) == ((2208988800 + 1792281600) << 32) | 0x40000000 == model.timetag(t2026)
    for t in (1.0e9 + 1.0 / 3.0, 1792300000.123456):
        assert capi.osc_timetag(t) == model.timetag(t)


PREFIX_CASES = [("/Aud/A", 5), ("/Audio/A", 95), ("/Audio/A", 9999990), ("/Audio/A", 0)]


@pytest.mark.parametrize("max_bytes", [96, 176, 1472])
@pytest.mark.parametrize("prefix,first", PREFIX_CASES)
def test_prefix_encoder_equals_the_model(fx, prefix, first, max_bytes):
    capi = fx.capi
    sizes = set()
    for guess in (1, 3, 40):                    # K depends on the longest message, which depends on n: take the counts around every K met
        try:
            sizes |= set(_counts(capi.osc_bundle_plan(capi.osc_stride(prefix, first, guess), 10 ** 6, max_bytes)[0]))
        except fx.FxError:
            pass
    if (prefix, first) == ("/Aud/A", 5):
        sizes.add(12)                           # "/Aud/A9" -> "/Aud/A10": 72 -> 76 bytes inside one bundle
    sizes.add(1)
    checked = 0
    for n in sorted(sizes):
        v = _vectors(n, seed=n)
        addresses = ["%s%d" % (prefix, first + c) for c in range(n)]
        try:
            model.plan(max(len(model.message(a, [0] * 12)) for a in addresses), n, max_bytes)
        except ValueError:                      # (an 84-byte message in a 96-byte datagram)
            with pytest.raises(fx.FxError):
                capi.osc_encode_bundles(prefix, first, v, TAG, max_bytes)
            continue
        out, lengths = capi.osc_encode_bundles(prefix, first, v, TAG, max_bytes)
        _check_against_model(fx, out, lengths, addresses, v, max_bytes)
        checked += 1
    assert checked or max_bytes == 96           # (96 bytes hold one message of 76 bytes, and none of 80)


def test_element_length_changes_inside_a_bundle(fx):
    capi = fx.capi
    v = _vectors(12, seed=5)
    out, lengths = capi.osc_encode_bundles("/Aud/A", 5, v, TAG, 1472)
    assert out.shape[0] == 1 and lengths[0] == 16 + 5 * (4 + 72) + 7 * (4 + 76)
    _, elements = model.parse(out[0, :lengths[0]])
    assert [len(e) for e in elements] == [72] * 5 + [76] * 7
    # a wider stride than the plan's: the same datagrams, more zeros
    wide, wide_n = capi.osc_encode_bundles("/Aud/A", 5, v, TAG, 1472, stride=out.shape[1] + 8)
    assert np.array_equal(wide_n, lengths) and np.array_equal(wide[:, :out.shape[1]], out) and not wide[:, out.shape[1]:].any()


def _address_sets(n):
    fill = "Mixer/Drums/Kick_0123456789-ABCDEFGHIJKLMNOPQRSTUVWXYZ~!#"
    def make(length, c):
        return "/" + "".join(fill[(c * 7 + k) % len(fill)] for k in range(length - 1))
    return {"1..8": [make(1 + c % 8, c) for c in range(n)], "1/124": [make(124 if c % 2 else 1, c) for c in range(n)]}


@pytest.mark.parametrize("which", ["1..8", "1/124"])
@pytest.mark.parametrize("max_bytes", [212, 408, 1472])
def test_addressed_encoder_equals_the_model(fx, which, max_bytes):
    capi = fx.capi
    sizes = set()
    for guess in (1, 2, 40):
        addresses = _address_sets(guess)[which]
        try:
            sizes |= set(_counts(capi.osc_bundle_plan(max(capi.osc_address_bytes(a) for a in addresses), 10 ** 6, max_bytes)[0]))
        except fx.FxError:
            pass
    checked = 0
    for n in sorted(sizes):
        addresses = _address_sets(n)[which]
        v = _vectors(n, seed=100 + n)
        out, lengths = capi.osc_encode_bundles_addressed(addresses, v, TAG, max_bytes)
        _check_against_model(fx, out, lengths, addresses, v, max_bytes)
        checked += 1
    assert checked >= 3


def test_encoders_refuse_bad_arguments(fx):
    capi = fx.capi
    L = fx.load_library()
    v = _vectors(4)
    fp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out = np.full((4, 2048), 0xA5, np.uint8)
    op = out.ctypes.data_as(ctypes.c_void_p)
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 4, fp, TAG, 95, op, 2048, None) == -1          # does not hold one message
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 4, fp, TAG, 65508, op, 2048, None) == -1
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 4, fp, TAG, 1472, op, 332, None) == -1         # stride below 16 + 4 * 80
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 4, fp, TAG, 1472, op, 338, None) == -1         # no multiple of 4
    assert L.fx_osc_encode_bundles(b"/Audio/A", -1, 4, fp, TAG, 1472, op, 2048, None) == -1
    assert L.fx_osc_encode_bundles(None, 0, 4, fp, TAG, 1472, op, 2048, None) == -1
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 0, fp, TAG, 1472, op, 2048, None) == 0
    bad = capi.c_strings(["/a", "b", "/c", "/d"])
    assert L.fx_osc_encode_bundles_addressed(bad, 4, fp, TAG, 1472, op, 2048, None) == -1
    assert b"track 1" in L.fx_last_error()
    assert (out == 0xA5).all()
    assert L.fx_osc_encode_bundles(b"/Audio/A", 0, 4, fp, TAG, 1472, op, 336, None) == 1          # lengths may be NULL
    assert (out.ravel()[336:] == 0xA5).all()


def _wait(receiver, key, want, seconds=5.0, stats="stats"):
    deadline = time.monotonic() + seconds
    got = getattr(receiver, stats)()[key]
    while got < want and time.monotonic() < deadline:
        time.sleep(0.002)
        got = getattr(receiver, stats)()[key]
    return got


@pytest.mark.parametrize("gro", [True, False])
def test_loopback_sender_to_bundle_receiver(fx, gro):
    capi = fx.capi
    C = 1000
    v = _vectors(C, seed=9)
    tag = capi.osc_timetag(1792281600.25)
    out, lengths = capi.osc_encode_bundles("/Audio/A", 0, v, tag, 1472)
    K, bundles, _ = capi.osc_bundle_plan(76, C, 1472)
    assert K == 18 and out.shape[0] == bundles == 56
    rx = capi.OscReceiver(prefix="/Audio/A", keep_channels=C, gro=gro, bundles=True)
    tx = capi.OscSender("127.0.0.1:%d" % rx.port)
    try:
        tx.update(out, lengths)
        assert tx.send() == bundles                                 # one fx_osc_sender_send
        assert _wait(rx, "datagrams", bundles) == bundles
        assert _wait(rx, "elements", C, stats="bundle_stats") == C
        st, bs = rx.stats(), rx.bundle_stats()
        assert st["datagrams"] == bundles and st["malformed"] == 0 and st["bytes"] == int(lengths.sum())
        assert bs == {"bundles": bundles, "elements": C, "last_timetag": tag}
        for c in (0, 17, 18, 999):
            assert rx.last(c) == fx.osc_encode("/Audio/A%d" % c, v[c]), c
        # plain messages to the same receiver are counted as before, and replace what the bundles left
        v2 = _vectors(C, seed=10)
        d, n = capi.osc_encode_batch("/Audio/A", 0, v2)
        tx.update(d, n)
        assert tx.send() == C
        assert _wait(rx, "datagrams", bundles + C) == bundles + C
        st = rx.stats()
        assert st["malformed"] == 0 and rx.bundle_stats()["bundles"] == bundles
        assert rx.last(17) == fx.osc_encode("/Audio/A17", v2[17])
    finally:
        tx.close()
        rx.close()


def test_receiver_without_the_flag_is_as_before(fx):
    capi = fx.capi
    v = _vectors(20, seed=11)
    out, lengths = capi.osc_encode_bundles("/Audio/A", 0, v, TAG, 1472)
    rx = capi.OscReceiver(prefix="/Audio/A", keep_channels=20)
    tx = capi.OscSender("127.0.0.1:%d" % rx.port)
    try:
        tx.update(out, lengths)
        assert tx.send() == 2
        assert _wait(rx, "datagrams", 2) == 2
        assert rx.stats()["malformed"] == 2                         # not a twelve-float message: what it said before bundles existed
        assert rx.bundle_stats() == {"bundles": 0, "elements": 0, "last_timetag": 0}
        assert rx.last(3) == b""
    finally:
        tx.close()
        rx.close()


def test_sink_publishes_bundles(fx):
    sharded = __import__("importlib").import_module("feature-extractor_amd.sharded")
    C = 100
    v = _vectors(C, seed=12)
    rx = fx.capi.OscReceiver(prefix="/Audio/A", keep_channels=C, bundles=True)
    sink = sharded.OscSink(None, "127.0.0.1:%d" % rx.port, bundle_bytes=1472)
    try:
        bundles = fx.capi.osc_bundle_plan(76, C, 1472)[1]
        assert sink.send(v) == bundles
        assert _wait(rx, "elements", C, stats="bundle_stats") == C
        assert rx.bundle_stats()["last_timetag"] == 1 and rx.stats()["malformed"] == 0
        assert rx.last(99) == fx.osc_encode("/Audio/A99", v[99])
    finally:
        sink.close()
        rx.close()


NEW_ENTRIES = ["fx_osc_bundle_plan", "fx_osc_timetag", "fx_osc_encode_bundles", "fx_osc_encode_bundles_addressed", "fx_get_osc_bundles",
               "fx_get_osc_bundles_addressed", "fx_osc_receiver_get_bundle_stats"]


def test_header_and_library_agree(fx):
    header = open(os.path.join(ROOT, "include", "fx.h")).read()
    L = fx.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in fx.capi.EXPORTS
        assert getattr(L, name) is not None                         # exported by the library
    assert "#define FX_ABI_VERSION 6" in header and L.fx_abi_version() == 6 == fx.capi.ABI_VERSION
    for define in ("#define FX_OSC_BUNDLE_MAX_ELEMENTS 1024", "#define FX_OSC_TIMETAG_IMMEDIATE 1", "#define FX_OSC_RECEIVER_BUNDLES 2u"):
        assert define in header, define
    kernels_h = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "FX_LAUNCH_OSC_BUNDLE = 13" in kernels_h and fx.capi.LAUNCH_KINDS[13] == "osc_bundle"
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_osc_bundle.hip" in build.SOURCES and "fx_osc_bundle.hip" not in build.HOST_SOURCES
