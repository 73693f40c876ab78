"""The RTP reorder window (include/fx.h, fx_rtp_set_window / fx_rtp_get_window) without a GPU: the C ABI declares and exports the
entries and refuses bad arguments before any device use; the window model (tests/rtp_window_model.py) is today's model at W = 0,
equals a receiver that resubmits early packets to today's model, does not depend on the arrival schedule, lets the most recent
packet win, drops a stream's holdings with its cursor, and does what the definition says at n > W, W = 1 and for a packet longer
than the span; and fx_rtp_place_span of csrc/fx_rtp_packet.h gives the model's placement on the host under AddressSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtp_model as rm
import rtp_window_model as wm
import rtp_window_traffic as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
CHANS = [1, 2, 5]


def models(B, W, first, kinds=(wm.Model,)):
    out = []
    for kind in kinds:
        m = kind(B, CHANS, sum(CHANS))
        rows = [(s, j) for s, K in enumerate(CHANS) for j in range(K)]
        m.set_sources(range(len(rows)), [r[0] for r in rows], [r[1] for r in rows])
        m.set_timestamps(range(len(CHANS)), first)
        if kind is wm.Model:
            m.set_window(W)
        out.append(m)
    return out


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ("fx_rtp_set_window", "fx_rtp_get_window"):
        assert name + "(" in text and name in fx.capi.EXPORTS and hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    assert "FX_RTP_PLACED = 1, FX_RTP_LATE = 2, FX_RTP_EARLY = 4, FX_RTP_MALFORMED = 8, FX_RTP_IGNORED = 16, FX_RTP_HELD = 32 }" in text
    assert "#define FX_RTP_MAX_WINDOW 65536" in text and "typedef struct fx_rtp_window_stats { long long held, recovered; } fx_rtp_window_stats;" in text
    assert fx.capi.RTP_HELD == wm.HELD == 32 and fx.capi.RTP_MAX_WINDOW == wm.MAX_WINDOW == 65536
    assert fx.capi.RTP_WINDOW_STATS_FIELDS == wm.WINDOW_STATS
    unit = open(os.path.join(CSRC, "fx_rtp.hip")).read()
    header = open(os.path.join(CSRC, "fx_rtp_packet.h")).read()
    assert "FX_RTP_BIT_HELD = 32" in header and "fx_rtp_place_span(" in header and "fx_rtp_place_span(" in unit
    assert "12 + 4" not in unit and "(int) (T - cursor)" not in unit       # the header arithmetic is stated once, in the header
    assert "sockets and the jitter-buffer policy" not in text


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    fake = ctypes.create_string_buffer(1 << 16)         # a zeroed block stands in for a context without an RTP unit (tests/test_rtp_cpu.py)
    got = ctypes.c_int(7)
    room = (ctypes.c_longlong * 8)()

    def refused(status, why):
        assert status == INVALID and why in lib.fx_last_error(), (why, status, lib.fx_last_error())

    refused(lib.fx_rtp_set_window(None, 48), b"null context")
    refused(lib.fx_rtp_set_window(fake, -1), b"window -1")
    refused(lib.fx_rtp_set_window(fake, 65537), b"window 65537")
    refused(lib.fx_rtp_set_window(fake, 1 << 30), b"a reorder window is 0 (none) to 65536")
    for window in (0, 1, 480, 65536):
        refused(lib.fx_rtp_set_window(fake, window), b"not configured")
    refused(lib.fx_rtp_get_window(None, ctypes.byref(got), room), b"null context")
    refused(lib.fx_rtp_get_window(fake, ctypes.byref(got), room), b"not configured")
    refused(lib.fx_rtp_get_window(fake, None, None), b"not configured")
    assert got.value == 7


@pytest.mark.parametrize("B", [2, 3])
def test_without_a_window_the_model_is_todays_model(fx, B):
    """randomised ticks: packets that run past their tick, come again, overlap, are cut short or belong to a stream that does not run"""
    rng = np.random.default_rng(20 + B)
    new, old = wm.Model(B, CHANS, 8), rm.Model(B, CHANS, 8)
    for m in (new, old):
        m.set_sources(range(8), [0, 1, 1, 2, 2, 2, -1, 2], [0, 0, 1, 0, 4, 4, 0, 2])
        m.set_timestamps([0, 2], [0xFFFFFF00, 77])                                  # stream 1 does not run
    kept = None
    for n in (1, 37, 480, 600, 5, 64):
        x = wt.samples(rng, sum(CHANS), n + 9, B)
        slots, lengths, stream_of = fx.rtp.packetise(x, CHANS, int(rng.choice([1, 6, 48])), [new.cursor[0], 5, new.cursor[2] + 2], bytes_per_sample=B)
        order = rng.permutation(len(lengths))[:max(1, len(lengths) - 1)]
        slots, lengths, stream_of = slots[order], lengths[order].copy(), stream_of[order]
        lengths[0] -= 1
        if kept is not None:
            width = max(slots.shape[1], kept[0].shape[1])
            pad = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])))
            slots, lengths, stream_of = np.concatenate([pad(kept[0]), pad(slots)]), np.concatenate([kept[1], lengths]), np.concatenate([kept[2], stream_of])
        got, want = new.tick(slots, lengths, stream_of, n), old.tick(slots, lengths, stream_of, n)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and not (got[1] & wm.HELD).any()
        assert np.array_equal(new.stats, old.stats) and new.cursor == old.cursor
        early = (want[1] & rm.EARLY) != 0
        early[-3:] = True                                   # and three that will be late, whatever they were
        kept = (slots[early], lengths[early], stream_of[early])
    assert old.stats[:, 2].sum() > 0 and old.stats[:, 3].sum() > 0 and old.stats[:, 1].sum() >= 6 and old.stats[1, 2:].sum() == 0
    w = new.window_dict()
    assert w["window"] == 0 and not w["held"].any() and not w["recovered"].any()


def jittered(rng, B, W, n, ticks, per_packet, first, fx, overlap=False):
    """a timeline of `ticks` ticks of n as packets, and a schedule that delivers each 0 .. W - m ahead of its sample time"""
    x = wt.samples(rng, sum(CHANS), n * ticks, B)
    packets = wt.packets_of(fx.rtp, x, CHANS, per_packet, first, B)
    position, m = packets[3], packets[4]
    if overlap:                                             # every fifth packet once more, three sample times on and with other bytes
        again = np.arange(0, len(m), 5)
        slots = packets[0][again].copy()
        stamps = (fx.rtp.timestamps_of(slots) + 3) & 0xFFFFFFFF
        slots[:, 4:8] = np.frombuffer(stamps.astype(">u4").tobytes(), np.uint8).reshape(-1, 4)
        slots[:, 12:] ^= 0x5A
        packets = (np.concatenate([packets[0], slots]),) + tuple(np.concatenate([p, p[again] + (3 if k == 2 else 0)]) for k, p in enumerate(packets[1:]))
    keep = packets[3] + packets[4] <= n * ticks             # (a shifted copy may run past the last tick)
    packets = tuple(p[keep] for p in packets)
    position, m = packets[3], packets[4]
    ahead = rng.integers(0, np.maximum(W - m, 0) + 1)
    arrival = wt.tick_of(np.maximum(position - ahead, 0), [n] * ticks)
    return x, packets, arrival


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("W,n,per_packet", [(48, 48, [6, 48, 1]), (100, 37, [48, 6, 6]), (7, 20, [1, 6, 6]), (480, 100, [48, 48, 6])])
def test_a_window_equals_resubmitting_early_packets_to_todays_model(fx, B, W, n, per_packet):
    """no packet reaches beyond the span of the tick it is submitted in; some overlap.  The merged definition, fed every packet again
    until it is no longer EARLY, gives the window model's blocks and counts."""
    rng = np.random.default_rng(B * 1000 + W)
    first = [0xFFFFFFF0, 5, 0x7FFFFFFF]
    ticks = 9
    _, packets, arrival = jittered(rng, B, W, n, ticks, per_packet, first, fx, overlap=True)
    assert wt.whole_in_span(packets[3], packets[4], arrival, [n] * ticks, W).all()
    windowed, = models(B, W, first)
    plain, = models(B, 0, first, kinds=(rm.Model,))
    carried, resubmitted, held = None, 0, 0
    for k in range(ticks):
        slots, lengths, stream_of = wt.submit(packets, arrival, k, order=rng.permutation if k % 2 else None)
        got, disposition = windowed.tick(slots, lengths, stream_of, n)
        held += int(((disposition & wm.HELD) != 0).sum())
        want, _, carried = wt.resubmitting(plain, slots, lengths, stream_of, n, carried)
        resubmitted += len(carried[1])
        assert got.tobytes() == want.tobytes(), k
        assert np.array_equal(windowed.stats[:, 4:], plain.stats[:, 4:]) and windowed.cursor == plain.cursor
    assert held > 0 and resubmitted >= held and windowed.recovered.sum() > 0
    assert not windowed.stats[:, 2:4].any()                 # nothing was lost to the window model
    assert not windowed.stats[:, 5].any()


@pytest.mark.parametrize("B", [2, 3])
def test_the_arrival_schedule_does_not_matter_without_overlaps(fx, B):
    first = [0xFFFFFF80, 0, 123456]
    W, n, ticks, per_packet = 96, 40, 8, [6, 48, 1]
    blocks = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        x, packets, arrival = jittered(np.random.default_rng(7), B, W, n, ticks, per_packet, first, fx)
        if seed == 3:                                       # on time: every packet in the tick of its first sample time
            arrival = wt.tick_of(packets[3], [n] * ticks)
        else:
            arrival = wt.tick_of(np.maximum(packets[3] - rng.integers(0, W - packets[4] + 1), 0), [n] * ticks)
        model, = models(B, W, first)
        out = [model.tick(*wt.submit(packets, arrival, k, order=rng.permutation), n)[0] for k in range(ticks)]
        blocks.append(np.concatenate([b.reshape(sum(CHANS), n, B) for b in out], axis=1))
        assert not model.stats[:, 5].any()
    assert blocks[0].tobytes() == blocks[1].tobytes() == blocks[2].tobytes()
    assert blocks[0].reshape(sum(CHANS), -1).tobytes() == rm.little_endian_bytes(x, B).tobytes()


def test_the_packages_schedule_helpers_cut_a_list_into_the_ticks_of_a_schedule(fx):
    """rtp.arrival_ticks / rtp.cut_into_ticks (what tools/rtp_ingest.py feeds a window with): a packet 0 .. W - m ahead lies whole in
    the span of its tick, a tick's packets keep the list's order, and the model hears the timeline back"""
    B, W, n, ticks, first = 3, 96, 40, 8, [0xFFFFFFF0, 9, 77]
    rng = np.random.default_rng(4)
    x = wt.samples(rng, sum(CHANS), n * ticks, B)
    packets = wt.packets_of(fx.rtp, x, CHANS, [6, 48, 1], first, B)
    assert np.array_equal(fx.rtp.timestamps_of(packets[0]), (np.asarray(first)[packets[2]] + packets[3]) & 0xFFFFFFFF)
    ahead = rng.integers(0, W - packets[4] + 1)
    arrival = fx.rtp.arrival_ticks(packets[3], ahead, n)
    assert np.array_equal(arrival, wt.tick_of(np.maximum(packets[3] - ahead, 0), [n] * ticks))
    assert wt.whole_in_span(packets[3], packets[4], arrival, [n] * ticks, W).all() and arrival.min() == 0 and (arrival < wt.tick_of(packets[3], [n] * ticks)).any()
    cut = fx.rtp.cut_into_ticks(packets[0], packets[1], packets[2], arrival, ticks)
    assert len(cut) == ticks and sum(len(c[1]) for c in cut) == len(arrival)
    model, = models(B, W, first)
    blocks = []
    for k, (slots, lengths, stream_of) in enumerate(cut):
        want = wt.submit(packets, arrival, k)
        assert slots.tobytes() == want[0].tobytes() and np.array_equal(lengths, want[1]) and np.array_equal(stream_of, want[2])
        blocks.append(model.tick(slots, lengths, stream_of, n)[0].reshape(sum(CHANS), n, B))
    assert np.concatenate(blocks, axis=1).reshape(sum(CHANS), -1).tobytes() == rm.little_endian_bytes(x, B).tobytes()
    assert fx.rtp.cut_into_ticks(packets[0][:0], [], [], []) == [] and len(fx.rtp.cut_into_ticks(packets[0][:0], [], [], [], 3)) == 3
    with pytest.raises(ValueError):
        fx.rtp.cut_into_ticks(packets[0], packets[1], packets[2], arrival[:-1])
    with pytest.raises(ValueError):
        fx.rtp.cut_into_ticks(packets[0], packets[1], packets[2], arrival - 1)


def one_stream(W, cursor=100, B=2, K=1):
    model = wm.Model(B, [K], K)
    model.set_sources(range(K), [0] * K, range(K))
    model.set_timestamps([0], [cursor])
    model.set_window(W)
    return model


def packet(T, values, B=2):
    """a mono packet whose samples are `values`"""
    body = b"".join(int(v).to_bytes(B, "big") for v in values)
    return bytes([0x80, 96, 0, 0]) + (T & 0xFFFFFFFF).to_bytes(4, "big") + bytes(4) + body


def tick(model, packets, n, fx):
    slots, lengths = fx.rtp.slots_of(packets)
    block, disposition = model.tick(slots, lengths, [0] * len(packets), n)
    return [int.from_bytes(bytes(block[0, 2 * q:2 * q + 2]), "little") for q in range(n)], list(disposition)


def test_the_most_recent_packet_wins(fx):
    model = one_stream(8)
    # tick 0, positions 0 .. 3 and the span to 11: a (index 0) and b (index 1) overlap at 6 .. 7 beyond the tick
    got, disposition = tick(model, [packet(104, [1] * 4), packet(106, [2] * 4)], 4, fx)
    assert got == [0] * 4 and disposition == [wm.HELD, wm.HELD] and model.window_dict()["held"][0] == 6
    # tick 1 (cursor 104): c covers 105 .. 106, held by a and by b, and wins both; the rest comes out of the held state
    got, disposition = tick(model, [packet(105, [3] * 2)], 4, fx)
    assert got == [1, 3, 3, 2] and disposition == [wm.PLACED]
    assert model.window_dict()["held"][0] == 2 and model.recovered[0] == 2
    # tick 2 (cursor 108): what b left, then nothing; a held position is overwritten by a later tick's HELD packet before its turn
    got, disposition = tick(model, [packet(113, [4] * 2)], 4, fx)
    assert got == [2, 2, 0, 0] and disposition == [wm.HELD]
    got, disposition = tick(model, [packet(114, [5] * 3), packet(110, [6])], 1, fx)          # cursor 112; 110 is late
    assert got == [0] and disposition == [wm.HELD, wm.LATE] and model.window_dict()["held"][0] == 4
    got, _ = tick(model, [], 4, fx)                         # cursor 113: 4 from tick 2, then 5 5 5 from the tick after
    assert got == [4, 5, 5, 5]
    assert model.stats[0].tolist() == [6, 0, 1, 0, 10, 7] and model.recovered[0] == 8 and not model.window_dict()["held"].any()


def test_a_cursor_change_drops_only_that_streams_holdings(fx):
    B = 3
    model, = models(B, 50, [10, 20, 30])
    x = wt.samples(np.random.default_rng(1), sum(CHANS), 60, B)
    packets = wt.packets_of(fx.rtp, x, CHANS, [6, 6, 6], [10, 20, 30], B)
    model.tick(packets[0], packets[1], packets[2], 20)      # everything at once: 40 positions a stream are held
    assert model.window_dict()["held"].tolist() == [40, 40, 40]
    model.set_timestamps([1], [40])                         # the same cursor: its holdings go all the same
    assert model.window_dict()["held"].tolist() == [40, 0, 40]
    block, _ = model.tick(packets[0][:0], [], [], 20)
    want = rm.little_endian_bytes(x[:, 20:40], B).reshape(sum(CHANS), 20, B).copy()
    want[1:3] = 0
    assert block.tobytes() == want.tobytes() and model.recovered.tolist() == [20, 0, 20]
    model.set_window(50)                                    # the same window: everything held goes, and the count of the recovered
    assert not model.window_dict()["held"].any() and not model.recovered.any()


def test_a_tick_longer_than_the_window_a_window_of_one_and_a_packet_longer_than_the_span(fx):
    # n > W: everything held is consumed, and the whole carry is new
    model = one_stream(3)
    got, disposition = tick(model, [packet(100, range(1, 9))], 4, fx)           # 8 sample times into a span of 7
    assert got == [1, 2, 3, 4] and disposition == [wm.PLACED | wm.HELD | wm.EARLY] and model.window_dict()["held"][0] == 3
    got, disposition = tick(model, [packet(110, [9, 9, 9]), packet(113, [7])], 5, fx)          # cursor 104, span 104 .. 111
    assert got == [5, 6, 7, 0, 0] and disposition == [wm.HELD | wm.EARLY, wm.EARLY]
    assert model.stats[0].tolist() == [3, 0, 0, 1, 7, 2] and model.window_dict()["held"][0] == 2 and model.recovered[0] == 3
    # W = 1
    model = one_stream(1)
    got, disposition = tick(model, [packet(102, [8]), packet(103, [9])], 2, fx)
    assert got == [0, 0] and disposition == [wm.HELD, wm.EARLY]
    got, disposition = tick(model, [], 2, fx)
    assert got == [8, 0] and model.recovered[0] == 1 and model.stats[0].tolist() == [2, 0, 0, 1, 1, 3]
    # the placement alone, wrap and far side included
    assert wm.place(100, 100, 8, 4, 3) == (0, 0, 7, wm.PLACED | wm.HELD | wm.EARLY)
    assert wm.place(99, 100, 20, 4, 3) == (-1, 0, 7, wm.LATE | wm.PLACED | wm.HELD | wm.EARLY)
    assert wm.place(107, 100, 2, 4, 3) == (7, 0, 0, wm.EARLY) and wm.place(106, 100, 1, 4, 3) == (6, 6, 7, wm.HELD)
    assert wm.place(5, 0xFFFFFFFE, 4, 4, 8) == (7, 7, 11, wm.HELD) and wm.place(0x80000000, 0, 4, 4, 8)[3] == wm.LATE
    for T, cursor, m, n in [(100, 100, 8, 4), (96, 100, 6, 10), (108, 100, 6, 10), (99, 100, 12, 10), (0x10, 0xFFFFFFC0, 48, 200)]:
        assert wm.place(T, cursor, m, n, 0) == rm.place(T, cursor, m, n)


def host_cases():
    cases = []
    for cursor in (0, 1000, 0x7FFFFFF0, 0x80000000, 0xFFFFFFC0, 0xFFFFFFFF):
        for off in (-(1 << 31), -(1 << 31) + 1, -70000, -65, -1, 0, 1, 63, 199, 200, 201, 679, 680, 681, 65735, 65736, 70000, (1 << 31) - 65537, (1 << 31) - 2, (1 << 31) - 1):
            for m in (1, 6, 48, 341, 10922, 21845, 32768):                      # up to 65536 / F for F = 192, 6, 3 and 2
                for n, W in ((1, 0), (200, 0), (200, 1), (1, 480), (200, 480), (600, 480), (200, 65536), ((1 << 31) - 1 - 65536, 65536)):
                    cases.append(((cursor + off) & 0xFFFFFFFF, cursor, m, n, W))
    return cases


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_place_span_on_the_host_sanitized_gives_the_models_placement(tmp_path):
    exe = str(tmp_path / "rtp_window_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    p = subprocess.run(cmd + [os.path.join(ROOT, "tests", "cpp", "rtp_window_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-3000:]
    cases = host_cases()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-500:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "%d cases" % len(cases) and len(lines) == len(cases) + 1
    seen = set()
    for line, case in zip(lines, cases):
        f = line.split()
        assert f[0] == "s" and tuple(int(v) for v in f[1:6]) == case, line
        got = tuple(int(v) for v in f[6:10])
        assert got == wm.place(*case), (line, wm.place(*case))
        if case[4] == 0:                                    # and fx_rtp_place says the same (its range is empty unless PLACED, as here)
            old = rm.place(*case[:4])
            assert f[10] == "=" and tuple(int(v) for v in f[11:15]) == got and (got[0], got[3]) == (old[0], old[3]) and (got[1:3] == old[1:3] or not got[3] & rm.PLACED), line
        seen.add(got[3])
    assert {wm.HELD, wm.PLACED | wm.HELD, wm.LATE | wm.PLACED | wm.HELD | wm.EARLY, wm.HELD | wm.EARLY, wm.LATE, wm.EARLY} <= seen
