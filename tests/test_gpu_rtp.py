"""fx_push_rtp on the GPU (include/fx.h, "RTP audio in"): the block, the disposition bytes, the statistics and the cursors equal the
model (tests/rtp_model.py) byte for byte, and everything after the unpack equals a twin context fed fx_push_samples with the model's
block -- raw, smoothed, pending samples, launches.  Shapes: a 256-point window (hops of 128), 70 tracks (two tiles of tracks, one
partial) on 5 streams of 1, 2, 8, 3 and 64 channels, ticks of 1 / 63 / 64 / 65 / 200 samples (a partial, a whole and two tiles of
positions), packets of 1 / 6 / 48 / 64 sample times."""
import ctypes

import numpy as np
import pytest

import dispatch_paths as dp
import rtp_model as rm

pytestmark = pytest.mark.gpu

N, C = 256, 70
CHANS = [1, 2, 8, 3, 64]
ROWS = sum(CHANS)
NS = [1, 63, 64, 65, 200]
MS = [1, 6, 48, 64]
FIRST = [0, 1000, 0xFFFFFFC0, 0x7FFFFFF0, 123456789]
EXTREMES = {2: [-0x8000, 0x7FFF, -1, 0, 1, 0x0102, -0x0102], 3: [-0x800000, 0x7FFFFF, -1, 0, 1, 0x010203, -0x010203]}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def samples(rng, n, B, rows=ROWS):
    x = rng.integers(-(1 << (8 * B - 1)), 1 << (8 * B - 1), (rows, n), dtype=np.int64)
    ext = EXTREMES[B]
    for k, v in enumerate(ext[:n]):                     # the extremes in every row, each row at another place
        x[:, k] = v
    return np.stack([np.roll(r, i) for i, r in enumerate(x)])


def sources(seed):
    """(tracks, stream, channel) for set_rtp_sources: every track in scrambled order, some on none, some streams heard twice, and a
    few tracks listed twice (the last entry wins)"""
    rng = np.random.default_rng(seed)
    tracks = rng.permutation(C)
    stream = rng.integers(-1, len(CHANS), C)
    stream[:8] = 4                                      # (the 64-channel stream is heard by several neighbours)
    channel = np.array([0 if s < 0 else rng.integers(0, CHANS[s]) for s in stream])
    again = rng.integers(0, C, 6)
    tracks = np.concatenate([tracks, tracks[again]])
    stream = np.concatenate([stream, rng.integers(-1, len(CHANS), 6)])
    channel = np.concatenate([channel, [0 if s < 0 else rng.integers(0, CHANS[s]) for s in stream[C:]]])
    return tracks, stream, channel


def make(gpu_fx, B, seed=1, first=FIRST, twin=False):
    an = gpu_fx.BatchAnalyser(C, N)
    an.rtp_configure("l16" if B == 2 else "l24", CHANS)
    model = rm.Model(B, CHANS, C)
    t, s, j = sources(seed)
    an.set_rtp_sources(t, s, j)
    model.set_sources(t, s, j)
    got = an.rtp_sources()
    assert same(got["stream"], model.stream) and same(got["channel"], model.channel)
    an.set_rtp_timestamps(range(len(CHANS)), first)
    model.set_timestamps(range(len(CHANS)), first)
    return (an, model, gpu_fx.BatchAnalyser(C, N)) if twin else (an, model)


def as_block(u8, B):
    """the model's block uint8 [C][n * B] as push_samples takes it"""
    return np.ascontiguousarray(u8).view(np.int16) if B == 2 else np.ascontiguousarray(u8)


def check_state(an, model):
    st = an.rtp_stats()
    for k, name in enumerate(rm.STATS):
        assert same(st[name], model.stats[:, k]), (name, st[name], model.stats[:, k])
    t, running = an.rtp_timestamps()
    assert list(running) == [int(r) for r in model.running]
    assert [int(v) for v, r in zip(t, model.running) if r] == [c for c, r in zip(model.cursor, model.running) if r]


def tick(an, model, slots, lengths, stream_of, n, B, twin=None, device=False):
    """one tick into the library and the model; block, disposition and (with a twin) the analysis compared -> the block"""
    if device:
        import torch
        got = an.push_rtp(torch.from_numpy(np.ascontiguousarray(slots)).cuda(), lengths, stream_of, n)
        got = tuple(g.cpu().numpy() for g in got)
    else:
        got = an.push_rtp(slots, lengths, stream_of, n)
    want_block, want_disposition = model.tick(slots, lengths, stream_of, n)
    block = an.rtp_block()
    assert block.view(np.uint8).reshape(C, -1).tobytes() == want_block.tobytes()
    assert same(got[2], want_disposition), (got[2], want_disposition)
    if twin is not None:
        launches = an.last_launches()
        want = twin.push_samples(as_block(want_block, B), sample_format="s24" if B == 3 else None)
        assert got[0].shape == want[0].shape and same(got[0], want[0]) and same(got[1], want[1])
        assert an.pending_samples() == twin.pending_samples()
        assert launches[0]["kind"] == "rtp" and launches[0]["T"] == n and launches[1:] == twin.last_launches(), launches
    return want_block


@pytest.mark.parametrize("B", [2, 3])
def test_block_disposition_and_stats_equal_the_model_over_the_matrix(gpu_fx, B):
    """every (n, m) as one tick of a running context.  Each tick's packets are cut from n + 5 samples, so its last packets run past
    the tick (EARLY); they are submitted again with the next tick, where they are part LATE and lie under that tick's own packets of
    other content (the greatest index wins); one packet of every tick is lost, one arrives twice, one is cut short (MALFORMED)."""
    an, model = make(gpu_fx, B)
    rng = np.random.default_rng(B)
    kept = None
    for n in NS:
        for m in MS:
            x = samples(rng, n + 5, B)
            slots, lengths, stream_of = gpu_fx.rtp.packetise(x, CHANS, m, model.cursor, bytes_per_sample=B)
            P = len(lengths)
            order = [i for i in range(P) if i != P // 3] + [P // 2]
            slots, lengths, stream_of = slots[order], lengths[order].copy(), stream_of[order]
            lengths[1] -= 1
            if kept is not None:                        # the last tick's packets that ran past it, in front: part late, and overwritten
                width = max(slots.shape[1], kept[0].shape[1])
                pad = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])))
                slots, lengths, stream_of = np.concatenate([pad(kept[0]), pad(slots)]), np.concatenate([kept[1], lengths]), np.concatenate([kept[2], stream_of])
            before = list(model.cursor)
            tick(an, model, slots, lengths, stream_of, n, B)
            check_state(an, model)
            early = [i for i in range(len(lengths))
                     if (p := rm.parse(bytes(slots[i, :lengths[i]]), CHANS[stream_of[i]] * B)) and rm.place(p[0], before[stream_of[i]], p[2], n)[3] & rm.EARLY]
            kept = (slots[early], lengths[early], stream_of[early])
    st = an.rtp_stats()
    assert st["malformed"].sum() == len(NS) * len(MS) and st["samples_missing"].sum() > 0 and st["early_packets"].sum() > 0
    an.close()


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("device", [False, True])
def test_analysis_equals_the_twin_fed_the_models_block(gpu_fx, B, device):
    """ticks whose length is no multiple of the hop, among them one of several hops and one that completes none"""
    an, model, twin = make(gpu_fx, B, seed=2, twin=True)
    rng = np.random.default_rng(10 + B)
    for n, m in [(200, 48), (63, 6), (65, 64), (480, 48), (1, 1), (700, 64)]:
        x = samples(rng, n, B) // 4
        slots, lengths, stream_of = gpu_fx.rtp.packetise(x, CHANS, m, model.cursor, bytes_per_sample=B)
        keep = rng.random(len(lengths)) > 0.1
        tick(an, model, slots[keep], lengths[keep], stream_of[keep], n, B, twin=twin, device=device)
    assert same(an.get_features(), twin.get_features())
    check_state(an, model)
    an.close(); twin.close()


def touching(slots, lengths, stream_of, cursor, n, B):
    """the packets that cover a position of the tick [cursor, cursor + n) of their stream"""
    keep = []
    for i in range(len(lengths)):
        T, _, m = rm.parse(bytes(slots[i, :lengths[i]]), CHANS[stream_of[i]] * B)
        if rm.place(T, cursor[stream_of[i]], m, n)[3] & rm.PLACED:
            keep.append(i)
    return keep


@pytest.mark.parametrize("B", [2, 3])
def test_cutting_invariance(gpu_fx, B):
    """1 000 samples as one tick, and as ticks of 137 / 480 / 383 with every packet submitted in each tick it touches"""
    first = [0xFFFFFE00, 5, 0x7FFFFF00, 0xFFFFFFFF, 42]
    x = samples(np.random.default_rng(3), 1000, B)
    slots, lengths, stream_of = gpu_fx.rtp.packetise(x, CHANS, 48, first, bytes_per_sample=B)
    an, model = make(gpu_fx, B, seed=3, first=first)
    whole = tick(an, model, slots, lengths, stream_of, 1000, B)
    an.close()
    an, model = make(gpu_fx, B, seed=3, first=first)
    parts, resubmitted = [], 0
    for n in (137, 480, 383):
        keep = touching(slots, lengths, stream_of, model.cursor, n, B)
        resubmitted += len(keep)
        parts.append(tick(an, model, slots[keep], lengths[keep], stream_of[keep], n, B).reshape(C, n, B))
    assert resubmitted > len(lengths)                   # some packets lie across a cut
    assert np.concatenate(parts, axis=1).tobytes() == whole.reshape(C, 1000, B).tobytes()
    an.close()


@pytest.mark.parametrize("B", [2, 3])
def test_order_loss_and_silence(gpu_fx, B):
    rng = np.random.default_rng(4)
    n = 200
    x = samples(rng, n, B) // 4
    an, model, twin = make(gpu_fx, B, seed=4, twin=True)
    slots, lengths, stream_of = gpu_fx.rtp.packetise(x, CHANS, 6, model.cursor, bytes_per_sample=B)
    # shuffled: no two packets disagree, so the order does not matter
    order = rng.permutation(len(lengths))
    full = tick(an, model, slots[order], lengths[order], stream_of[order], n, B, twin=twin)
    straight = rm.Model(B, CHANS, C)
    straight.set_sources(range(C), model.stream, model.channel)
    straight.set_timestamps(range(len(CHANS)), FIRST)
    assert straight.tick(slots, lengths, stream_of, n)[0].tobytes() == full.tobytes()
    # 20 % lost: zeros exactly at the lost packets' positions
    x2 = samples(rng, n, B) // 4
    slots, lengths, stream_of = gpu_fx.rtp.packetise(x2, CHANS, 6, model.cursor, bytes_per_sample=B)
    lost = rng.random(len(lengths)) < 0.2
    cursor = list(model.cursor)
    got = tick(an, model, slots[~lost], lengths[~lost], stream_of[~lost], n, B, twin=twin).reshape(C, n, B)
    hole = np.zeros((len(CHANS), n), bool)
    for i in np.flatnonzero(lost):
        T, _, m = rm.parse(bytes(slots[i, :lengths[i]]), CHANS[stream_of[i]] * B)
        d0 = rm.signed32(T - cursor[stream_of[i]])
        hole[stream_of[i], d0:d0 + m] = True
    assert hole.any()
    for c in range(C):
        s, j = int(model.stream[c]), int(model.channel[c])
        if s >= 0:
            row = sum(CHANS[:s]) + j
            want = np.where(hole[s][:, None], 0, rm.little_endian_bytes(x2[row:row + 1], B).reshape(n, B))
            assert same(got[c], want), c
        else:
            assert not got[c].any()
    # no packets at all: a zero block, analysed as silence
    empty = np.zeros((0, 12), np.uint8)
    for k in (300, 1):
        assert not tick(an, model, empty, [], [], k, B, twin=twin).any()
    assert same(an.get_features(), twin.get_features())
    check_state(an, model)
    an.close(); twin.close()


@pytest.mark.parametrize("B", [2, 3])
def test_wrap_and_header_variants(gpu_fx, B):
    """stream 2's cursor is 0xFFFFFFC0 and the first tick is 200 samples: it crosses 2^32 at position 64; then every header variant"""
    an, model = make(gpu_fx, B, seed=5)
    rng = np.random.default_rng(5)
    x = samples(rng, 200, B)
    tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B), 200, B)
    assert model.cursor[2] == 0x88
    for csrc in (0, 1, 15):
        for ext in (None, 0, 3):
            for pad in (0, 1, 2, 3):
                x = samples(rng, 13, B)
                tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 6, model.cursor, csrc=csrc, extension_words=ext, padding=pad, bytes_per_sample=B), 13, B)
    st = an.rtp_stats()
    assert not st["malformed"].any() and not st["samples_missing"].any()
    check_state(an, model)
    an.close()


def test_malformed_classes_and_streams_that_do_not_run(gpu_fx):
    B = 3
    an = gpu_fx.BatchAnalyser(C, N)
    an.rtp_configure("l24", CHANS)
    model = rm.Model(B, CHANS, C)
    t, s, j = sources(6)
    an.set_rtp_sources(t, s, j); model.set_sources(t, s, j)
    an.set_rtp_timestamps([1, 4], [7, 7]); model.set_timestamps([1, 4], [7, 7])        # streams 0, 2 and 3 do not run
    F = CHANS[1] * B
    good = bytes([0x80, 96, 0, 0]) + (7).to_bytes(4, "big") + bytes(4) + bytes(range(1, 1 + 2 * F))
    ext = bytes([0x90]) + good[1:12] + b"\xbe\xde\x00\x09" + bytes(2 * F)
    packets = [good, good[:11], b"", bytes([0x40]) + good[1:], bytes([0x82]) + good[1:16], bytes([0x90]) + good[1:14], ext, good[:12], good + b"\x01",
               bytes([0xA0]) + good[1:-1] + b"\x00", bytes([0xA0]) + good[1:-1] + b"\x0d", bytes([0xA0]) + good[1:12] + bytes(5) + b"\x06"]
    slots, lengths = gpu_fx.rtp.slots_of(packets)
    stream_of = np.ones(len(packets), np.int32)
    slots = np.concatenate([slots, slots[:1], slots[1:2]])        # and the good and a bad one on a stream that does not run
    lengths = np.concatenate([lengths, lengths[:1], lengths[1:2]])
    stream_of = np.concatenate([stream_of, [0, 2]]).astype(np.int32)
    got = an.push_rtp(slots, lengths, stream_of, 10)
    want_block, want = model.tick(slots, lengths, stream_of, 10)
    assert list(want) == [rm.PLACED] + [rm.MALFORMED] * 11 + [rm.IGNORED, rm.MALFORMED]
    assert same(got[2], want) and an.rtp_block().tobytes() == want_block.tobytes()
    slots0, lengths0 = gpu_fx.rtp.slots_of([good[:12] + bytes(B * 4)])
    got = an.push_rtp(slots0, lengths0, [0], 10)
    want_block, want = model.tick(slots0, lengths0, [0], 10)
    assert list(want) == [rm.IGNORED] and same(got[2], want) and not an.rtp_block().any()
    check_state(an, model)
    an.close()


def test_a_source_change_zeroes_the_pending_samples(gpu_fx):
    B = 2
    an, model, twin = make(gpu_fx, B, seed=7, twin=True)
    rng = np.random.default_rng(7)
    x = samples(rng, 100, B) // 4
    tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B), 100, B, twin=twin)
    assert an.pending_samples() == 100
    same_source = (int(model.stream[5]), int(model.channel[5]))
    an.set_rtp_sources([3, 5, 3], [0, same_source[0], 4], [0, same_source[1], 63])      # track 5: nothing changes, cleared all the same
    model.set_sources([3, 5, 3], [0, same_source[0], 4], [0, same_source[1], 63])
    twin.clear_pending_channels([3, 5])
    assert an.pending_samples() == 100 and an.rtp_sources()["stream"][3] == 4 and an.rtp_sources()["channel"][3] == 63
    x = samples(rng, 300, B) // 4
    tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B), 300, B, twin=twin)
    assert same(an.get_features(), twin.get_features())
    # the unit is the slot's: a reset of the analysers keeps sources, cursors and statistics
    an.reset_state(); twin.reset_state()
    check_state(an, model)
    x = samples(rng, 200, B) // 4
    tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B), 200, B, twin=twin)
    an.close(); twin.close()


def test_refused_ticks_change_nothing_and_configure_starts_over(gpu_fx):
    B = 3
    an, model, twin = make(gpu_fx, B, seed=8, twin=True)
    rng = np.random.default_rng(8)
    x = samples(rng, 100, B) // 4
    slots, lengths, stream_of = gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B)
    tick(an, model, slots, lengths, stream_of, 100, B, twin=twin)
    for bad_lengths, bad_streams, why in [(np.r_[lengths[:-1], slots.shape[1] + 1], stream_of, "lengths[%d]" % (len(lengths) - 1)),
                                          (np.r_[-1, lengths[1:]], stream_of, "lengths[0]"),
                                          (lengths, np.r_[stream_of[:2], 5, stream_of[3:]], "stream_of[2] = 5"),
                                          (lengths, np.r_[-1, stream_of[1:]], "stream_of[0] = -1")]:
        with pytest.raises(gpu_fx.FxError, match=why.replace("[", r"\[").replace("]", r"\]")):
            an.push_rtp(slots, bad_lengths, bad_streams, 100)
        assert an.last_launches() == [] and an.pending_samples() == 100
    # fx_push_samples' own refusal: fp32 samples are pending in the twin's place of an RTP context
    other = gpu_fx.BatchAnalyser(C, N)
    other.rtp_configure("l24", CHANS)
    other.push_samples(np.zeros((C, 100), np.float32))
    with pytest.raises(gpu_fx.FxError):
        other.push_rtp(slots, lengths, stream_of, 100)
    assert other.last_launches() == [] and other.pending_samples() == 100 and not other.rtp_stats()["packets"].any()
    other.close()
    check_state(an, model)
    # the capacity too small: refused, and the length reported
    n_out, room = ctypes.c_int(0), (ctypes.c_ubyte * 16)()
    assert an._lib.fx_rtp_get_block(an._h, room, 16, ctypes.byref(n_out), None, gpu_fx.capi.MEM_HOST) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT and n_out.value == 100
    x = samples(rng, 100, B) // 4
    tick(an, model, *gpu_fx.rtp.packetise(x, CHANS, 48, model.cursor, bytes_per_sample=B), 100, B, twin=twin)
    # configured again: not running, no sources, statistics zero; with no streams: gone
    an.rtp_configure("l16", [2, 2])
    st = an.rtp_stats()
    assert all(not st[k].any() for k in rm.STATS) and not an.rtp_timestamps()[1].any() and (an.rtp_sources()["stream"] == -1).all()
    an.rtp_configure("l16", [])
    with pytest.raises(gpu_fx.FxError, match="not configured"):
        an.push_rtp(slots, lengths, stream_of, 100)
    an.close(); twin.close()


def test_a_context_without_rtp_launches_what_it_always_launched(gpu_fx):
    rows = {r.id: r for r in dp.ROWS}
    for rid in ("block-batch-1024-s16", "block-hop-1024-s16"):
        r = rows[rid]
        assert r.entry == "samples" and not r.hooks and not r.tuning and r.fmt == "s16"
        an = gpu_fx.BatchAnalyser(r.C, r.N)
        x = np.random.default_rng(9).integers(-8000, 8000, (r.C, 16 * r.N // 2)).astype(np.int16)     # (the launches do not depend on the samples)
        at, H = 0, r.N // 2
        for n in [r.per[0]] + [r.per[1]] * 4:
            frames = (an.pending_samples() + n) // H
            an.push_samples(np.ascontiguousarray(x[:, at:at + n]))
            at += n
            got = an.last_launches()
            assert all(l["kind"] != "rtp" for l in got) and got == r.expect[frames], (rid, n, got)
        an.close()
