"""Per-track OSC addresses without a GPU (ref AnalyserTrackController.h:17,22-23: every track's (ip, secondaryIP, bundle);
OSCFeatureAnalysisOutput.h:107: sender.send (bundleAddress, ...)): fx_osc_encode_addressed, the host twin of
fx_get_osc_datagrams_addressed, against the per-message encoder and the oracle's; every class of invalid address refused with the
track named; the new entries declared, exported and bound with the ABI number unmoved; the word-forming function of the device
kernel (csrc/fx_osc_words.h) run on the host under ASan + UBSan by a stand-alone program (tests/cpp/osc_table_host.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import osc_address_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
ENTRIES = ("fx_set_osc_addresses", "fx_osc_address_stride", "fx_get_osc_datagrams_addressed", "fx_osc_encode_addressed", "fx_osc_sender_set_routes")


def test_entries_are_declared_exported_and_bound(fx):
    header = open(os.path.join(ROOT, "include", "fx.h")).read()
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in header and name in fx.capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define FX_OSC_ADDRESS_MAX 124" in header and fx.capi.OSC_ADDRESS_MAX == 124
    assert lib.fx_abi_version() == 6 and fx.capi.ABI_VERSION == 6 and "#define FX_ABI_VERSION 6" in header     # additive: the ABI number does not move
    for method in ("set_osc_addresses", "osc_datagrams", "osc_address_stride"):
        assert callable(getattr(fx.BatchAnalyser, method)), method
    assert callable(fx.capi.OscSender.set_routes) and fx.capi.LAUNCH_KINDS[12] == "osc_table"
    hpp = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    batch = hpp[hpp.index("class OSCBatchSender"):hpp.index("class LiveAnalyser")]
    assert "void setBundleAddresses (" in batch and "void setRoutes (" in batch
    # each entry cites the reference lines it stands for
    for name in ENTRIES[:4]:
        doc = header[:header.index(name + "(")].rsplit("/*", 1)[1]
        assert "AnalyserTrackController.h:17" in doc or "OSCFeatureAnalysisOutput.h:107" in doc, name
    assert "AnalyserTrackController.h:17,22-23" in header[:header.index("fx_osc_sender_set_routes(")].rsplit("/*", 1)[1]


def test_the_unit_is_built_for_gfx950_and_the_host_units_name_no_symbol_of_it(fx):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_osc_table.hip" in build.SOURCES and any(u[0] == "fx_osc_table.hip" for u in build.UNITS)
    assert "fx_osc_table.hip" not in build.HOST_SOURCES
    fx.load_library()
    blob = open(fx.library_path(), "rb").read()
    assert b"fx_osc_table_kernel" in blob and b"gfx950" in blob
    for source in build.HOST_SOURCES:
        text = open(os.path.join(CSRC, source)).read()
        for name in ENTRIES[:3] + ("fx_osc_table_kernel", "launch_osc_table_kernel", "OscTableParams", "struct fx_osc_table {"):
            assert name not in text, (source, name)


@pytest.mark.parametrize("offset", [0, 5, 11])
def test_addressed_encoder_is_the_per_message_encoder(fx, oracle, offset):
    """Every message = fx_osc_encode = the oracle's message, for addresses of 1 .. 124 bytes (every residue mod 4, both ends), with
    NaN, +-inf and -0.0 among the values; at the smallest stride and at 12 bytes more, the slots' remainders zero."""
    capi = fx.capi
    n = 2 * len(cases.LENGTHS) + 3
    addr = cases.addresses(n, offset)
    assert sorted(set(len(a) for a in addr)) == cases.LENGTHS
    v = cases.vectors(n, seed=offset)
    assert np.isnan(v).any() and np.isinf(v).any() and np.signbit(v[-1, 0])
    smallest = max(cases.message_bytes(a) for a in addr)
    assert smallest == 192 and smallest % 4 == 0
    for stride in (smallest, smallest + 12):
        d, lengths = capi.osc_encode_addressed(addr, v, stride=stride)
        assert d.shape == (n, stride)
        for c in range(n):
            want = oracle.osc_message(addr[c], v[c])
            assert lengths[c] == len(want) == cases.message_bytes(addr[c]), c
            assert bytes(d[c, :lengths[c]]) == want == fx.osc_encode(addr[c], v[c]), (c, addr[c])
            assert not d[c, lengths[c]:].any(), c                   # the rest of the slot is zeros
    d0, n0 = capi.osc_encode_addressed(addr, v)                      # stride None: the smallest
    assert d0.shape == (n, smallest) and np.array_equal(n0, lengths)
    # short addresses alone: the smallest stride follows the table
    d1, n1 = capi.osc_encode_addressed(["/a", "/abc"], v[:2])
    assert d1.shape == (2, 72) and list(n1) == [68, 72] and not d1[0, 68:].any()
    # the reference's own default bundle address and a mixer path
    for a in ("/Audio/Features", "/Mixer/Drums/Kick"):
        d2, n2 = capi.osc_encode_addressed([a], v[:1])
        assert bytes(d2[0, :n2[0]]) == oracle.osc_message(a, v[0])


def test_addressed_encoder_refuses_strides_and_counts(fx):
    capi = fx.capi
    lib = fx.load_library()
    addr = cases.addresses(6)
    v = cases.vectors(6)
    smallest = max(cases.message_bytes(a) for a in addr)
    for stride in (smallest - 4, smallest + 2, smallest + 1, 0, -4):
        with pytest.raises(fx.FxError):
            capi.osc_encode_addressed(addr, v, stride=stride)
    out = np.zeros((6, smallest), np.uint8)
    ptrs = capi.c_strings(addr)
    fp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.fx_osc_encode_addressed(ptrs, -1, fp, out.ctypes.data_as(ctypes.c_void_p), smallest, None) == -1
    assert lib.fx_osc_encode_addressed(None, 6, fp, out.ctypes.data_as(ctypes.c_void_p), smallest, None) == -1
    assert lib.fx_osc_encode_addressed(ptrs, 6, None, out.ctypes.data_as(ctypes.c_void_p), smallest, None) == -1
    assert lib.fx_osc_encode_addressed(ptrs, 6, fp, None, smallest, None) == -1
    assert not out.any()
    assert lib.fx_osc_encode_addressed(ptrs, 0, fp, out.ctypes.data_as(ctypes.c_void_p), smallest, None) == 0
    assert lib.fx_osc_encode_addressed(ptrs, 6, fp, out.ctypes.data_as(ctypes.c_void_p), smallest, None) == 6      # lengths may be NULL


BAD = [("", "empty"), ("Audio/A", "start with '/'"), ("/Audio A", "0x21"), ("/Audio/\x7f", "0x21"), ("/" + "x" * 124, "124"),
       ("/Audio/\xe9", "0x21"), ("/tab\there", "0x21")]


@pytest.mark.parametrize("bad, why", BAD)
@pytest.mark.parametrize("track", [0, 3, 6])
def test_every_invalid_address_class_is_refused_naming_the_track(fx, bad, why, track):
    """empty, no leading '/', a space, 0x7F, 125 bytes (and a byte above 0x7E, a control byte): the whole call fails, fx_last_error names
    the track and the output is untouched."""
    lib = fx.load_library()
    addr = [a.encode() for a in cases.addresses(7)]
    addr[track] = bad.encode("latin-1")
    v = cases.vectors(7)
    out = np.full((7, 192), 0xEE, np.uint8)
    lengths = np.full(7, -7, np.int32)
    got = lib.fx_osc_encode_addressed(fx.capi.c_strings(addr), 7, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.ctypes.data_as(ctypes.c_void_p), 192,
                                      lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    message = lib.fx_last_error().decode()
    assert got == -1 and ("track %d:" % track) in message and why in message, message
    assert (out == 0xEE).all() and (lengths == -7).all()
    with pytest.raises(fx.FxError, match="track %d:" % track):
        fx.capi.osc_encode_addressed(addr, v)


def test_context_entries_refuse_a_null_context_before_device_use(fx):
    lib = fx.load_library()
    inv = fx.capi.FX_ERR_INVALID_ARGUMENT
    out = np.zeros(192, np.uint8)
    assert lib.fx_set_osc_addresses(None, None) == inv and b"null context" in lib.fx_last_error()
    assert lib.fx_osc_address_stride(None) == -1
    assert lib.fx_get_osc_datagrams_addressed(None, out.ctypes.data_as(ctypes.c_void_p), 192, None, 0) == inv
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)             # no context: the count is checked before any use of it
    an.num_channels = 4
    with pytest.raises(ValueError, match=r"one OSC address per track \(4\), not 3"):
        an.set_osc_addresses(["/a", "/b", "/c"])
    an._h = None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_word_forming_function_on_the_host_sanitized(tmp_path):
    """csrc/fx_osc_words.h's osc_table_word -- the function every thread of fx_osc_table_kernel runs -- for every word of every track
    over the same address set, against fx_osc_encode; a stand-alone program under ASan + UBSan, no Python in the process."""
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    fake = os.path.join(ROOT, "tests", "cpp", "fake_hip")
    exe = str(tmp_path / "osc_table_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-I", fake, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(fake, "fake_hip.cpp"),
           os.path.join(ROOT, "tests", "cpp", "osc_table_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout, p.stdout[-2000:]
    words = int(p.stdout.split("words checked:")[1].split()[0])
    assert words == 71 * (192 + 204) // 4 * 2, p.stdout            # 71 tracks, strides 192 and 204, two sets of values
