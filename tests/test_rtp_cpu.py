"""RTP audio in (include/fx.h, fx_rtp_configure .. fx_push_rtp) without a GPU: the C ABI declares and exports the entries, they refuse
bad arguments before any device use, the host packetiser and the model (tests/rtp_model.py) agree byte for byte, the model does what
the definition says at the timestamp wrap, on overlapping, part-late and part-early packets and on every header variant, and the one
statement of the parser (csrc/fx_rtp_packet.h) gives the model's classes on the host under AddressSanitizer, without a read past a
datagram's length."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtp_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
ENTRIES = ("fx_rtp_configure", "fx_rtp_set_track_sources", "fx_rtp_get_track_sources", "fx_rtp_set_cursors", "fx_rtp_get_cursors",
           "fx_push_rtp", "fx_rtp_get_block", "fx_rtp_get_stats")
EXTREMES = {2: [-0x8000, 0x7FFF, -1, 0, 1, 0x0102, -0x0102], 3: [-0x800000, 0x7FFFFF, -1, 0, 1, 0x010203, -0x010203]}


def samples(rng, rows, n, B):
    """integer samples [rows][n] over the whole range of B bytes, the extremes among them"""
    x = rng.integers(-(1 << (8 * B - 1)), 1 << (8 * B - 1), (rows, n), dtype=np.int64)
    ext = EXTREMES[B]
    x.ravel()[:min(x.size, len(ext))] = ext[:x.size]
    return x


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    for word in ("FX_RTP_L16 = 0, FX_RTP_L24 = 1", "FX_RTP_PLACED = 1, FX_RTP_LATE = 2, FX_RTP_EARLY = 4, FX_RTP_MALFORMED = 8, FX_RTP_IGNORED = 16"):
        assert word in text
    assert (fx.capi.RTP_PLACED, fx.capi.RTP_LATE, fx.capi.RTP_EARLY, fx.capi.RTP_MALFORMED, fx.capi.RTP_IGNORED) == (rm.PLACED, rm.LATE, rm.EARLY, rm.MALFORMED, rm.IGNORED)
    assert fx.capi.RTP_STATS_FIELDS == rm.STATS
    for name in rm.STATS:
        assert name in text


def test_launch_kind_and_build_lists(fx):
    assert fx.capi.LAUNCH_KINDS[19] == "rtp"
    assert "constexpr int FX_LAUNCH_RTP = 19;" in open(os.path.join(CSRC, "fx_kernels.h")).read()
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_rtp.hip" in build.SOURCES and any(u[0] == "fx_rtp.hip" for u in build.UNITS) and "fx_rtp.hip" not in build.HOST_SOURCES
    assert "fx_rtp_packet.h" in build.HEADERS
    # the parser is stated once: the unit includes the header and carries no second copy of its arithmetic
    unit = open(os.path.join(CSRC, "fx_rtp.hip")).read()
    assert '#include "fx_rtp_packet.h"' in unit and "12 + 4" not in unit


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID, OK, HOST, DEVICE = fx.capi.FX_ERR_INVALID_ARGUMENT, fx.capi.FX_OK, fx.capi.MEM_HOST, fx.capi.MEM_DEVICE
    ints = (ctypes.c_int * 4)(1, 2, 3, 4)
    zeros = (ctypes.c_int * 4)(0, 0, 0, 0)
    stamps = (ctypes.c_uint * 4)()
    buf = (ctypes.c_ubyte * 256)()
    got = ctypes.c_int(7)
    # A zeroed block stands in for a context: each refusal below comes before the entry touches a device, and the zeroed context
    # has no RTP unit, which every entry but fx_rtp_configure says last of all
    fake = ctypes.create_string_buffer(1 << 16)

    def refused(status, why):
        assert status == INVALID and why in lib.fx_last_error(), (why, status, lib.fx_last_error())

    refused(lib.fx_rtp_configure(None, 0, 1, ints), b"null context")
    refused(lib.fx_rtp_configure(fake, 2, 1, ints), b"unknown payload format 2")
    refused(lib.fx_rtp_configure(fake, -1, 1, ints), b"unknown payload format")
    refused(lib.fx_rtp_configure(fake, 0, -1, ints), b"-1 streams")
    refused(lib.fx_rtp_configure(fake, 1, 65537, ints), b"65537 streams")
    refused(lib.fx_rtp_configure(fake, 0, 4, None), b"null channel counts")
    refused(lib.fx_rtp_configure(fake, 0, 4, zeros), b"channels[0] = 0")
    refused(lib.fx_rtp_configure(fake, 1, 4, (ctypes.c_int * 4)(1, 64, 65, 1)), b"channels[2] = 65")
    assert lib.fx_rtp_configure(fake, 0, 0, None) == OK                        # nothing to free is no error

    refused(lib.fx_rtp_set_track_sources(None, zeros, 1, zeros, zeros), b"null context")
    refused(lib.fx_rtp_set_track_sources(fake, zeros, -1, zeros, zeros), b"negative channel count")
    refused(lib.fx_rtp_set_track_sources(fake, None, 2, zeros, zeros), b"null channel list")
    refused(lib.fx_rtp_set_track_sources(fake, zeros, 2, None, zeros), b"null source list")
    refused(lib.fx_rtp_set_track_sources(fake, zeros, 2, zeros, None), b"null source list")
    refused(lib.fx_rtp_set_track_sources(fake, zeros, 2, zeros, zeros), b"not configured")
    assert lib.fx_rtp_set_track_sources(fake, None, 0, None, None) == OK      # an empty list is a no-op
    refused(lib.fx_rtp_get_track_sources(None, ints, ints), b"null context")
    refused(lib.fx_rtp_get_track_sources(fake, ints, ints), b"not configured")

    refused(lib.fx_rtp_set_cursors(None, zeros, 1, stamps), b"null context")
    refused(lib.fx_rtp_set_cursors(fake, zeros, -3, stamps), b"negative stream count")
    refused(lib.fx_rtp_set_cursors(fake, None, 1, stamps), b"null stream or timestamp list")
    refused(lib.fx_rtp_set_cursors(fake, zeros, 1, None), b"null stream or timestamp list")
    refused(lib.fx_rtp_set_cursors(fake, zeros, 1, stamps), b"not configured")
    assert lib.fx_rtp_set_cursors(fake, None, 0, None) == OK
    refused(lib.fx_rtp_get_cursors(None, stamps, ints), b"null context")
    refused(lib.fx_rtp_get_cursors(fake, stamps, ints), b"not configured")

    assert lib.fx_push_rtp(None, buf, ints, zeros, 1, 64, 48, HOST, None, None, ctypes.byref(got), None) == INVALID
    assert b"null context" in lib.fx_last_error() and got.value == 0
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    cases = [((buf, ints, zeros, 1, 64, -1, HOST), b"negative sample count"),
             ((buf, ints, zeros, -1, 64, 48, HOST), b"negative packet count"),
             ((buf, ints, zeros, 1, 64, 48, 7), b"unknown memory kind"),
             ((buf, ints, zeros, 1, 8, 48, HOST), b"slot stride 8"),
             ((buf, ints, zeros, 1, 14, 48, HOST), b"slot stride 14"),
             ((buf, ints, zeros, 1, 65540, 48, HOST), b"slot stride 65540"),
             ((None, ints, zeros, 1, 64, 48, HOST), b"null packets, lengths or stream list"),
             ((buf, None, zeros, 1, 64, 48, HOST), b"null packets, lengths or stream list"),
             ((buf, ints, None, 1, 64, 48, HOST), b"null packets, lengths or stream list"),
             ((odd, ints, zeros, 1, 64, 48, DEVICE), b"4-byte aligned"),
             ((buf, ints, zeros, 1, 64, 48, HOST), b"not configured"),
             ((None, None, None, 0, 64, 48, HOST), b"not configured")]
    for args, why in cases:
        got.value = 7
        refused(lib.fx_push_rtp(fake, *args, None, None, ctypes.byref(got), None), why)
        assert got.value == 0, why
    # nothing to do is no error
    assert lib.fx_push_rtp(fake, buf, ints, zeros, 1, 64, 0, HOST, None, None, None, None) == OK

    n = ctypes.c_int(7)
    refused(lib.fx_rtp_get_block(None, buf, 256, ctypes.byref(n), None, HOST), b"null context")
    assert n.value == 0
    refused(lib.fx_rtp_get_block(fake, None, 256, None, None, HOST), b"null output pointer")
    refused(lib.fx_rtp_get_block(fake, buf, 256, None, None, 9), b"unknown memory kind")
    refused(lib.fx_rtp_get_block(fake, buf, 256, None, None, HOST), b"not configured")
    refused(lib.fx_rtp_get_stats(None, buf), b"null context")
    refused(lib.fx_rtp_get_stats(fake, None), b"null output pointer")
    refused(lib.fx_rtp_get_stats(fake, buf), b"not configured")


@pytest.mark.parametrize("B", [2, 3])
def test_packetise_then_model_returns_the_planar_input(fx, B):
    rng = np.random.default_rng(B)
    chans = [1, 2, 8, 3, 64]
    for n, m in [(1, 1), (63, 6), (64, 48), (65, 64), (200, 48), (200, 1)]:
        x = samples(rng, sum(chans), n, B)
        first = [0, 1000, 0xFFFFFFC0, 0x7FFFFFF0, 123456789]
        slots, lengths, stream_of = fx.rtp.packetise(x, chans, m, first, bytes_per_sample=B)
        assert slots.shape[1] % 4 == 0 and slots.shape[0] == len(chans) * -(-n // m)
        model = rm.Model(B, chans, x.shape[0])
        rows = [(s, j) for s, K in enumerate(chans) for j in range(K)]
        model.set_sources(range(x.shape[0]), [r[0] for r in rows], [r[1] for r in rows])
        model.set_timestamps(range(len(chans)), first)
        block, disposition = model.tick(slots, lengths, stream_of, n)
        assert block.tobytes() == rm.little_endian_bytes(x, B).tobytes()
        assert (disposition == rm.PLACED).all()
        st = model.stats_dict()
        assert (st["packets"] == -(-n // m)).all() and (st["samples_placed"] == n).all() and not st["samples_missing"].any() and not st["malformed"].any()
        assert model.cursor == [(t + n) & 0xFFFFFFFF for t in first]


def one_stream(B, K, n, cursor, packets):
    """a model of one running stream of K channels heard by K tracks, ticked once with `packets` (bytes each) -> (block, disposition, model)"""
    model = rm.Model(B, [K], K)
    model.set_sources(range(K), [0] * K, range(K))
    model.set_timestamps([0], [cursor])
    width = max(12, (max([len(p) for p in packets] + [12]) + 3) & ~3)
    slots = np.zeros((len(packets), width), np.uint8)
    for i, p in enumerate(packets):
        slots[i, :len(p)] = np.frombuffer(p, np.uint8)
    block, disposition = model.tick(slots, [len(p) for p in packets], [0] * len(packets), n)
    return block, disposition, model


def packet(T, payload, first=0x80, csrc=0, ext=None, pad=0):
    head = bytes([first | (0x20 if pad else 0) | (0x10 if ext is not None else 0) | csrc, 96, 0, 0]) + (T & 0xFFFFFFFF).to_bytes(4, "big") + bytes(4)
    head += bytes(range(4 * csrc))
    if ext is not None:
        head += b"\xbe\xde" + ext.to_bytes(2, "big") + bytes([0xEE] * (4 * ext))
    return head + payload + (bytes(pad - 1) + bytes([pad]) if pad else b"")


def test_timestamp_wrap(fx):
    """cursor 0xFFFFFFC0, a tick of 200: the stream crosses 2^32 at position 64"""
    B, K, n, cursor = 3, 2, 200, 0xFFFFFFC0
    x = samples(np.random.default_rng(5), K, n, B)
    slots, lengths, stream_of = fx.rtp.packetise(x, [K], 48, [cursor], bytes_per_sample=B)
    stamps = [int.from_bytes(bytes(slots[i, 4:8]), "big") for i in range(len(lengths))]
    assert stamps == [0xFFFFFFC0, 0xFFFFFFF0, 0x20, 0x50, 0x80]
    model = rm.Model(B, [K], K)
    model.set_sources(range(K), [0] * K, range(K))
    model.set_timestamps([0], [cursor])
    block, disposition = model.tick(slots, lengths, stream_of, n)
    assert block.tobytes() == rm.little_endian_bytes(x, B).tobytes() and list(disposition) == [rm.PLACED] * 4 + [rm.PLACED]
    assert model.cursor == [0x88]
    assert rm.place(0x10, 0xFFFFFFC0, 48, 200)[:3] == (0x50, 0x50, 0x80)
    assert rm.place(0xFFFFFFB0, 0x20, 48, 200)[0] == -112


def test_the_greatest_index_wins_where_packets_overlap():
    """a test of the MODEL (tests/rtp_model.py) against the definition; the library is held to the model in tests/test_gpu_rtp.py"""
    B, K, n = 2, 1, 20
    a = packet(100, bytes([0x11, 0x11] * 10))           # positions 0 .. 9
    b = packet(105, bytes([0x22, 0x22] * 10))           # 5 .. 14
    c = packet(103, bytes([0x33, 0x33] * 4))            # 3 .. 6
    block, disposition, model = one_stream(B, K, n, 100, [a, b, c])
    want = [0x11] * 3 + [0x33] * 4 + [0x22] * 8 + [0] * 5
    assert list(block.reshape(n, 2)[:, 0]) == want and list(disposition) == [rm.PLACED] * 3
    assert model.stats_dict()["samples_placed"][0] == 15 and model.stats_dict()["samples_missing"][0] == 5
    block, _, _ = one_stream(B, K, n, 100, [c, b, a])   # the other order: a now covers c's and b's start
    assert list(block.reshape(n, 2)[:, 0]) == [0x11] * 10 + [0x22] * 5 + [0] * 5


def test_part_late_and_part_early_packets():
    """a test of the MODEL against the definition (the library: tests/test_gpu_rtp.py)"""
    B, K, n = 3, 1, 10
    body = lambda lo, m: b"".join(bytes([0, 0, v]) for v in range(lo, lo + m))
    late = packet(96, body(1, 6))                       # positions -4 .. 1: its last two are in the tick
    early = packet(108, body(11, 6))                    # 8 .. 13: its first two
    gone = packet(80, body(21, 6))                      # entirely late
    ahead = packet(110, body(31, 6))                    # entirely early: it starts at n
    both = packet(99, body(41, 12))                     # -1 .. 10: late and early and placed
    block, disposition, model = one_stream(B, K, n, 100, [late, early, gone, ahead])
    assert list(disposition) == [rm.LATE | rm.PLACED, rm.EARLY | rm.PLACED, rm.LATE, rm.EARLY]
    assert list(block.reshape(n, 3)[:, 0]) == [5, 6, 0, 0, 0, 0, 0, 0, 11, 12]
    st = model.stats_dict()
    assert (st["packets"][0], st["late_packets"][0], st["early_packets"][0], st["samples_placed"][0], st["samples_missing"][0]) == (4, 1, 1, 4, 6)
    block, disposition, _ = one_stream(B, K, n, 100, [both])
    assert list(disposition) == [rm.LATE | rm.EARLY | rm.PLACED] and list(block.reshape(n, 3)[:, 0]) == list(range(42, 52))
    # the early packet again with the next tick: its part before the new cursor is ignored
    block, disposition, _ = one_stream(B, K, n, 110, [early, ahead])
    assert list(disposition) == [rm.LATE | rm.PLACED, rm.PLACED] and list(block.reshape(n, 3)[:, 0]) == [31, 32, 33, 34, 35, 36, 0, 0, 0, 0]


@pytest.mark.parametrize("B", [2, 3])
def test_header_variants(fx, B):
    K, n = 3, 12
    x = samples(np.random.default_rng(11), K, n, B)
    want = rm.little_endian_bytes(x, B).tobytes()
    for csrc in (0, 1, 15):
        for ext in (None, 0, 3):
            for pad in (0, 1, 2, 3):
                slots, lengths, stream_of = fx.rtp.packetise(x, [K], 6, [77], csrc=csrc, extension_words=ext, padding=pad, bytes_per_sample=B)
                assert lengths[0] == 12 + 4 * csrc + (0 if ext is None else 4 + 4 * ext) + 6 * K * B + pad
                model = rm.Model(B, [K], K)
                model.set_sources(range(K), [0] * K, range(K))
                model.set_timestamps([0], [77])
                block, disposition = model.tick(slots, lengths, stream_of, n)
                assert block.tobytes() == want and (disposition == rm.PLACED).all(), (csrc, ext, pad)
                T, h, m = rm.parse(bytes(slots[1, :lengths[1]]), K * B)
                assert (T, h, m) == (83, 12 + 4 * csrc + (0 if ext is None else 4 + 4 * ext), 6)


def test_each_malformed_class():
    """a test of the MODEL's parser against the definition; the parser of csrc/fx_rtp_packet.h is held to it by the sanitized host
    program below, the kernel in tests/test_gpu_rtp.py"""
    F = 6
    good = packet(5, bytes(12))
    assert rm.parse(good, F) == (5, 12, 2)
    assert rm.parse(good[:11], F) is None and rm.parse(b"", F) is None                      # shorter than a header
    assert rm.parse(bytes([0x40]) + good[1:], F) is None                                    # version 1
    assert rm.parse(bytes([0xC0]) + good[1:], F) is None                                    # version 3
    assert rm.parse(packet(5, b"", csrc=2)[:16], F) is None                                 # the CSRC list runs past the end
    assert rm.parse(packet(5, b"", ext=0)[:14], F) is None                                  # no room for the extension's header
    assert rm.parse(packet(5, bytes(12), ext=9)[:40], F) is None                            # the extension runs past the end
    assert rm.parse(good[:12], F) is None                                                   # no payload
    assert rm.parse(packet(5, bytes(13)), F) is None                                        # not whole sample times
    assert rm.parse(bytes([0xA0]) + good[1:-1] + b"\x00", F) is None                        # padding of 0
    assert rm.parse(bytes([0xA0]) + good[1:-1] + b"\x0d", F) is None                        # padding that reaches into the header
    assert rm.parse(packet(5, b"", pad=6), F) is None                                       # nothing but padding
    assert rm.parse(packet(5, bytes(12), pad=6), F) == (5, 12, 2)
    # a packet of another stream's frame size
    assert rm.parse(packet(5, bytes(12)), 9) is None and rm.parse(packet(5, bytes(18)), 9) == (5, 12, 2)
    # a stream that is not running: valid packets are ignored, malformed ones are still malformed
    model = rm.Model(3, [2], 2)
    model.set_sources([0, 1], [0, 0], [0, 1])
    slots = np.zeros((2, 24), np.uint8)
    slots[0] = np.frombuffer(good, np.uint8)
    block, disposition = model.tick(slots, [24, 11], [0, 0], 4)
    assert list(disposition) == [rm.IGNORED, rm.MALFORMED] and not block.any()
    assert model.stats[0].tolist() == [1, 1, 0, 0, 0, 0] and model.cursor == [0]


def run_host_program(tmp_path, source, sanitize=True):
    exe = str(tmp_path / "rtp_packet_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-DRTP_HOST_COUNT_ONLY"])
    p = subprocess.run(cmd + [source, "-o", exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_parser_on_the_host_sanitized_gives_the_models_classes(tmp_path):
    out = run_host_program(tmp_path, os.path.join(ROOT, "tests", "cpp", "rtp_packet_host.cpp"))
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]             # (a sanitizer report ends the program with a status)
    lines = out.stdout.splitlines()
    assert lines[-1] == "2134 datagrams, 0 reads outside"
    valid = 0
    for line in lines[:-1]:
        f = line.split()
        if f[0] == "p":
            b = b"" if f[1] == "-" else bytes.fromhex(f[1])
            want = rm.parse(b, int(f[2]))
            got = None if f[3] == "M" else tuple(int(v) for v in f[3:6])
            assert got == want, line
            valid += got is not None
        else:
            T, cursor, m, n, d0, lo, hi, bits = (int(v) for v in f[1:])
            w0, wlo, whi, wbits = rm.place(T, cursor, m, n)
            assert (d0, bits) == (w0, wbits) and ((lo, hi) == (wlo, whi) if bits & rm.PLACED else lo == hi), line
    assert valid >= 100                                 # the patterns are not all refused
    assert sum(1 for l in lines if l.startswith("p")) == 22 * 97 and sum(1 for l in lines if l.startswith("q")) == 6 * 11 * 5 * 3 + 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_a_parser_that_trusts_the_extension_bit_is_caught(tmp_path):
    """the host check is not vacuous: a parser that asks for the extension's length before it knows those bytes exist reads outside a
    short datagram, and the program says so (here by its own count alone: built to touch nothing outside)"""
    header = open(os.path.join(CSRC, "fx_rtp_packet.h")).read()
    old = "        if (h + 4 > len) return false;\n"
    assert header.count(old) == 1
    (tmp_path / "fx_rtp_packet.h").write_text(header.replace(old, ""))
    src = open(os.path.join(ROOT, "tests", "cpp", "rtp_packet_host.cpp")).read()
    bad = tmp_path / "bad.cpp"
    bad.write_text(src.replace("../../feature-extractor_amd/csrc/", str(tmp_path) + "/"))
    out = run_host_program(tmp_path, str(bad), sanitize=False)
    assert out.returncode == 1 and " 0 reads outside" not in out.stdout.splitlines()[-1]
