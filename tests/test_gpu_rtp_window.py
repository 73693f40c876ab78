"""The RTP reorder window on the GPU (include/fx.h, "the RTP reorder window"): block, disposition bytes, statistics, window counters
and cursors equal the window model (tests/rtp_window_model.py) after every tick; the blocks and the analysis do not depend on the
arrival schedule; everything after the unpack equals a twin fed fx_push_samples with the model's blocks; and the state rules hold.
Shapes: a 1024-point context, 8 tracks on 3 streams of 1, 2 and 5 channels -- sample times of 2 / 4 / 10 bytes in L16 and 3 / 6 / 15
in L24, so ring offsets are odd and unaligned -- one track without a source, two on the same channel."""
import numpy as np
import pytest

import rtp_model as rm
import rtp_window_model as wm
import rtp_window_traffic as wt

pytestmark = pytest.mark.gpu

N, C = 1024, 8
CHANS = [1, 2, 5]
ROWS = sum(CHANS)
TRACKS = (list(range(C)), [0, 1, 1, 2, 2, 2, -1, 2], [0, 0, 1, 0, 4, 4, 0, 2])
FIRST = [0xFFFFFF00, 1000, 0x7FFFFFF0]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def make(gpu_fx, B, W, first=FIRST, twin=False):
    an = gpu_fx.BatchAnalyser(C, N)
    an.rtp_configure("l16" if B == 2 else "l24", CHANS)
    model = wm.Model(B, CHANS, C)
    an.set_rtp_sources(*TRACKS)
    model.set_sources(*TRACKS)
    an.set_rtp_timestamps(range(len(CHANS)), first)
    model.set_timestamps(range(len(CHANS)), first)
    if W is not None:
        an.rtp_set_window(W)
        model.set_window(W)
    return (an, model, gpu_fx.BatchAnalyser(C, N)) if twin else (an, model)


def check_state(an, model):
    st = an.rtp_stats()
    for k, name in enumerate(rm.STATS):
        assert same(st[name], model.stats[:, k]), (name, st[name], model.stats[:, k])
    got, want = an.rtp_window(), model.window_dict()
    assert got["window"] == want["window"]
    for name in wm.WINDOW_STATS:
        assert same(got[name], want[name]), (name, got[name], want[name])
    t, running = an.rtp_timestamps()
    assert list(running) == [int(r) for r in model.running]
    assert [int(v) for v, r in zip(t, model.running) if r] == [c for c, r in zip(model.cursor, model.running) if r]


def as_block(u8, B):
    return np.ascontiguousarray(u8).view(np.int16) if B == 2 else np.ascontiguousarray(u8)


def tick(an, model, slots, lengths, stream_of, n, B, twin=None, device=False):
    """one tick into the library and the model; block, disposition and (with a twin) the analysis compared -> (block, raw, smoothed)"""
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
    return want_block, got[0], got[1]


def traffic(gpu_fx, rng, B, W, ticks, per_packet, first, exact=False):
    """the ticks' timeline as packets and the tick each is submitted in.  exact: every packet 0 .. W - m ahead of its sample time, so
    whole in its span, none lost; else 0 .. W ahead (a packet may run past its span), a few late, a few twice (the copy a tick
    later), every seventh once more three sample times on with other bytes, stream 1 with a gap, and -1: never"""
    total = int(np.sum(ticks))
    x = wt.samples(rng, ROWS, total, B, scale=4)
    packets = wt.packets_of(gpu_fx.rtp, x, CHANS, per_packet, first, B)
    if exact:
        ahead = rng.integers(0, np.maximum(W - packets[4], 0) + 1)
        return x, packets, wt.tick_of(np.maximum(packets[3] - ahead, 0), ticks)
    again = np.arange(0, len(packets[1]), 7)
    other = packets[0][again].copy()
    stamps = (gpu_fx.rtp.timestamps_of(other) + 3) & 0xFFFFFFFF
    other[:, 4:8] = np.frombuffer(stamps.astype(">u4").tobytes(), np.uint8).reshape(-1, 4)
    other[:, 12:] ^= 0x5A
    twice = np.arange(3, len(packets[1]), 11)
    count = len(packets[1])
    packets = (np.concatenate([packets[0], other, packets[0][twice]]),) + tuple(np.concatenate([p, p[again] + (3 if k == 2 else 0), p[twice]]) for k, p in enumerate(packets[1:]))
    position, m = packets[3], packets[4]
    ahead = rng.integers(0, W + 1, len(m))
    late = rng.random(len(m)) < 0.04
    ahead[late] = -rng.integers(1, 80, int(late.sum()))
    arrival = wt.tick_of(np.maximum(position - ahead, 0), ticks)
    arrival[count + len(again):] += 1                       # the second copies
    arrival[(packets[2] == 1) & (position >= 300) & (position < 420)] = -1
    return x, packets, arrival


ORDERS = [None, lambda k: np.arange(k)[::-1], None, lambda k: np.random.default_rng(k).permutation(k)]


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("W", [1, 7, 48, 480, 1000])
def test_block_disposition_stats_window_and_cursors_equal_the_model_after_every_tick(gpu_fx, B, W):
    rng = np.random.default_rng(100 * B + W)
    ticks = np.concatenate([[480, 1, 37, 600], rng.choice([1, 37, 480, 600], 8)])
    per_packet = [[1, 6, 48], [48, 1, 6], [6, 48, 1]][W % 3]
    an, model = make(gpu_fx, B, W)
    _, packets, arrival = traffic(gpu_fx, rng, B, W, ticks, per_packet, FIRST)
    seen = 0
    for k, n in enumerate(ticks):
        slots, lengths, stream_of = wt.submit(packets, arrival, k, order=ORDERS[k % 4])
        lengths = lengths.copy()
        if len(lengths) > 2:
            lengths[2] -= 1                                 # MALFORMED
        tick(an, model, slots, lengths, stream_of, int(n), B)
        check_state(an, model)
        seen += len(lengths)
    st, w = an.rtp_stats(), an.rtp_window()
    assert seen > 100 and st["packets"].sum() + st["malformed"].sum() == seen and st["malformed"].sum() > 0
    assert w["recovered"].sum() > 0 and st["samples_missing"][1] > 50 and st["late_packets"].sum() > 0
    an.close()


@pytest.mark.parametrize("W,ticks", [(480, [100] * 12), (48, [480, 1, 37, 600] * 3)])
def test_the_stamps_tick_numbers_start_over_without_a_trace(gpu_fx, W, ticks):
    """test hook bit 7 (csrc/fx_kernels.h): the tick numbers in the stamps start over after every third tick, as they do after 2^32
    - 1 ticks.  Positions held across a restart -- at W = 480 and n = 100 every one is -- are still owned, and still lose to a later
    packet: the model, which knows no tick numbers, is matched after every tick."""
    B = 3
    rng = np.random.default_rng(W)
    an, model = make(gpu_fx, B, W)
    an.set_test_hooks(128)
    _, packets, arrival = traffic(gpu_fx, rng, B, W, ticks, [6, 48, 1], FIRST)
    for k, n in enumerate(ticks):
        tick(an, model, *wt.submit(packets, arrival, k, order=ORDERS[k % 4]), n, B)
        check_state(an, model)
    assert an.rtp_window()["recovered"].min() > 0
    an.close()


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("device", [False, True])
def test_blocks_and_analysis_do_not_depend_on_the_arrival_schedule(gpu_fx, B, device):
    """the same non-overlapping packets on time into one context and jittered, in another order, into another"""
    W, ticks = 480, [480, 37, 600, 480, 480, 1, 600]
    rng = np.random.default_rng(B)
    x, packets, jitter = traffic(gpu_fx, rng, B, W, ticks, [48, 6, 48], FIRST, exact=True)
    on_time = wt.tick_of(packets[3], ticks)
    assert (jitter != on_time).sum() > len(on_time) // 4
    out = []
    for arrival, order in ((on_time, None), (jitter, rng.permutation)):
        an, model = make(gpu_fx, B, W)
        got = [tick(an, model, *wt.submit(packets, arrival, k, order=order), n, B, device=device) for k, n in enumerate(ticks)]
        assert not an.rtp_stats()["samples_missing"].any()
        out.append((np.concatenate([g[0].reshape(C, -1, B) for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1),
                    np.concatenate([g[2] for g in got], axis=1), an.get_features()))
        an.close()
    for a, b in zip(*out):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert out[0][1].shape[1] == sum(ticks) // (N // 2) and out[1][0][0].tobytes() == rm.little_endian_bytes(x[:1], B).tobytes()


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("W", [48, 600])
def test_analysis_equals_the_twin_fed_the_models_blocks(gpu_fx, B, W):
    rng = np.random.default_rng(7 * B + W)
    ticks = [480, 600, 37, 480, 1, 600]
    an, model, twin = make(gpu_fx, B, W, twin=True)
    _, packets, arrival = traffic(gpu_fx, rng, B, W, ticks, [6, 48, 1], FIRST)
    for k, n in enumerate(ticks):
        tick(an, model, *wt.submit(packets, arrival, k, order=ORDERS[k % 4]), n, B, twin=twin)
    assert same(an.get_features(), twin.get_features()) and an.rtp_window()["recovered"].sum() > 0
    check_state(an, model)
    an.close(); twin.close()


@pytest.mark.parametrize("B", [2, 3])
def test_packets_held_across_the_timestamp_wrap(gpu_fx, B):
    """every cursor 100 below 2^32, W = 480: the first tick's span crosses the wrap, and its held packets land beyond it"""
    first = [0xFFFFFFFF - 99] * 3
    W, ticks = 480, [90, 200, 200, 90]
    an, model = make(gpu_fx, B, W, first=first)
    x, packets, arrival = traffic(gpu_fx, np.random.default_rng(B), B, W, ticks, [48, 6, 1], first, exact=True)
    whole = []
    for k, n in enumerate(ticks):
        whole.append(tick(an, model, *wt.submit(packets, arrival, k), n, B)[0].reshape(C, n, B))
        check_state(an, model)
        if k == 0:
            assert an.rtp_window()["held"].min() > 10 and model.cursor == [0xFFFFFFFF - 9] * 3
    assert model.cursor == [480] * 3 and an.rtp_window()["recovered"].min() > 100
    assert np.concatenate(whole, axis=1)[3].tobytes() == rm.little_endian_bytes(x[3:4], B).tobytes()
    an.close()


def test_state_rules(gpu_fx):
    B, W, n = 3, 200, 100
    rng = np.random.default_rng(5)
    an, model = make(gpu_fx, B, W)
    x = wt.samples(rng, ROWS, 6 * n, B)
    packets = wt.packets_of(gpu_fx.rtp, x, CHANS, [6, 48, 6], FIRST, B)
    arrival = wt.tick_of(np.maximum(packets[3] - 150, 0), [n] * 6)
    tick(an, model, *wt.submit(packets, arrival, 0), n, B)
    check_state(an, model)
    assert an.rtp_window()["held"].min() >= 150
    # a refused tick (a bad length entry) changes nothing, the held state included
    before = an.rtp_window()
    slots, lengths, stream_of = wt.submit(packets, arrival, 1)
    with pytest.raises(gpu_fx.FxError, match=r"lengths\[0\]"):
        an.push_rtp(slots, np.r_[slots.shape[1] + 1, lengths[1:]], stream_of, n)
    after = an.rtp_window()
    assert an.last_launches() == [] and all(same(before[k], after[k]) for k in before)
    tick(an, model, slots, lengths, stream_of, n, B)
    check_state(an, model)
    # a tick of no samples is a no-op: its packets are not looked at
    an.push_rtp(*wt.submit(packets, arrival, 2), 0)
    check_state(an, model)
    # a source change does not touch the held state: track 6 hears what stream 1 holds from its next tick on
    an.set_rtp_sources([6], [1], [1]); model.set_sources([6], [1], [1])
    check_state(an, model)
    # a new cursor drops what the listed stream holds, and only that
    held = an.rtp_window()["held"]
    assert held.min() > 0
    an.set_rtp_timestamps([1], [model.cursor[1]]); model.set_timestamps([1], [model.cursor[1]])
    assert an.rtp_window()["held"].tolist() == [held[0], 0, held[2]]
    block = tick(an, model, *wt.submit(packets, arrival, 2), n, B)[0].reshape(C, n, B)
    assert block[0].any() and block[3].any() and same(block[2], block[6])
    check_state(an, model)
    # the same window again: everything held goes, and the recovered count
    an.rtp_set_window(W); model.set_window(W)
    check_state(an, model)
    assert not an.rtp_window()["held"].any() and not an.rtp_window()["recovered"].any()
    tick(an, model, *wt.submit(packets, arrival, 3), n, B)
    check_state(an, model)
    # another window, then none
    an.rtp_set_window(7); model.set_window(7)
    tick(an, model, *wt.submit(packets, arrival, 4), n, B)
    check_state(an, model)
    with pytest.raises(gpu_fx.FxError, match="window 65537"):
        an.rtp_set_window(65537)
    assert an.rtp_window()["window"] == 7
    # configured again: no window, nothing held
    an.rtp_configure("l24", CHANS)
    w = an.rtp_window()
    assert w["window"] == 0 and not w["held"].any() and not w["recovered"].any()
    an.close()


@pytest.mark.parametrize("B", [2, 3])
def test_without_a_window_a_tick_is_the_tick_it_was(gpu_fx, B):
    """W = 0 after a window, W = 0 set outright and a context that never heard of the window: the same launch records, results,
    disposition bytes and statistics, tick by tick (against tests/rtp_model.py: today's definition)"""
    rng = np.random.default_rng(B)
    ticks = [480, 37, 600, 1]
    made = [make(gpu_fx, B, W) for W in (None, 0, 0)]
    made[2][0].rtp_set_window(48)
    made[2][0].rtp_set_window(0)
    plain = rm.Model(B, CHANS, C)
    plain.set_sources(*TRACKS)
    plain.set_timestamps(range(len(CHANS)), FIRST)
    _, packets, arrival = traffic(gpu_fx, rng, B, 0, ticks, [48, 6, 1], FIRST)
    for k, n in enumerate(ticks):
        slots, lengths, stream_of = wt.submit(packets, arrival, k)
        got = [an.push_rtp(slots, lengths, stream_of, n) + (an.last_launches(), an.rtp_block()) for an, _ in made]
        want_block, want_disposition = plain.tick(slots, lengths, stream_of, n)
        for g in got:
            assert same(g[0], got[0][0]) and same(g[1], got[0][1]) and same(g[2], want_disposition) and g[3] == got[0][3]
            assert g[4].view(np.uint8).reshape(C, -1).tobytes() == want_block.tobytes()
        assert got[0][3][0]["kind"] == "rtp" and not (want_disposition & wm.HELD).any()
    for an, _ in made:
        st = an.rtp_stats()
        assert all(same(st[name], plain.stats[:, j]) for j, name in enumerate(rm.STATS))
        assert an.rtp_window()["window"] == 0
        an.close()
