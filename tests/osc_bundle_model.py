"""An independent model of the OSC 1.0 bundles of include/fx.h (fx_osc_bundle_plan, fx_osc_encode_bundles*, fx_get_osc_bundles*):
a builder and a parser written with `struct` alone -- nothing of the package, no numpy.  Values travel as their 32-bit patterns, so
NaN payloads, infinities, -0.0 and denormals are compared as bits.

A bundle datagram: b"#bundle\\0", a 64-bit big-endian NTP time tag, then per element a big-endian int32 size and that many bytes.  An
element is a track's feature message (ref OSCFeatureAnalysisOutput.h:107): the address, NUL-terminated and zero-padded to a multiple
of 4; b",ffffffffffff\\0\\0\\0"; twelve big-endian float32 in wire order."""
import math
import struct

# wire position -> AudioFeatures slot: onset, rms, f0, centroid, slope, spread, flatness, ler, flux, her, oer, inharm
# (slots: onset 0, rms 1, f0 2, centroid 3, spread 4, flatness 5, ler 6, flux 7, slope 8, her 9, oer 10, inharm 11)
WIRE_SLOTS = (0, 1, 2, 3, 8, 4, 5, 6, 7, 9, 10, 11)
HEADER = b"#bundle\0"
TAGS = b",ffffffffffff\0\0\0"
MAX_ELEMENTS = 1024
MAX_DATAGRAM = 65507
IMMEDIATE = 1


def _raw(address):
    return address.encode("latin-1") if isinstance(address, str) else bytes(address)


def message(address, bits12):
    """the message of one track; bits12: the twelve values' uint32 patterns in AudioFeatures slot order"""
    a = _raw(address)
    a += b"\0" * (4 - len(a) % 4)
    return a + TAGS + struct.pack(">12I", *[int(bits12[s]) for s in WIRE_SLOTS])


def plan(longest, num_tracks, max_datagram_bytes):
    """(K, number of bundles, stride); ValueError where the library refuses"""
    if num_tracks < 1 or max_datagram_bytes > MAX_DATAGRAM:
        raise ValueError("no plan")
    K = min(num_tracks, MAX_ELEMENTS, (max_datagram_bytes - 16) // (4 + longest))
    if K < 1:
        raise ValueError("the datagram does not hold one message")
    return K, (num_tracks + K - 1) // K, 16 + K * (4 + longest)


def timetag(unix_seconds):
    ntp = unix_seconds + 2208988800.0
    whole = math.floor(ntp)
    return (int(whole) << 32) | int((ntp - whole) * 4294967296.0)


def bundles(messages, tag, max_datagram_bytes):
    """the datagrams of these messages (one per track, ascending), K and the stride"""
    K, count, stride = plan(max(len(m) for m in messages), len(messages), max_datagram_bytes)
    out = []
    for b in range(count):
        d = HEADER + struct.pack(">Q", tag)
        for m in messages[b * K:(b + 1) * K]:
            d += struct.pack(">i", len(m)) + m
        out.append(d)
    return out, K, stride


def parse(datagram):
    """(time tag, [element bytes]); ValueError for what a receiver counts as malformed"""
    d = bytes(datagram)
    if len(d) < 16 or d[:8] != HEADER:
        raise ValueError("no bundle header")
    tag, = struct.unpack(">Q", d[8:16])
    at, elements = 16, []
    while at < len(d):
        if len(d) - at < 4:
            raise ValueError("a size runs past the end")
        size, = struct.unpack(">i", d[at:at + 4])
        if size < 0 or size % 4 or size > len(d) - at - 4:
            raise ValueError("size %d at %d" % (size, at))
        e = d[at + 4:at + 4 + size]
        if e[:8] == HEADER:
            raise ValueError("nested bundle")
        if not is_feature_message(e):
            raise ValueError("an element is not a twelve-float message")
        elements.append(e)
        at += 4 + size
    if not elements:
        raise ValueError("empty bundle")
    return tag, elements


def is_feature_message(m):
    if len(m) < 68 or len(m) % 4 or m[:1] != b"/":
        return False
    apad = len(m) - 64
    a = m[:apad].split(b"\0", 1)[0]
    return len(a) < apad and (len(a) + 4) // 4 * 4 == apad and m[apad:apad + 16] == TAGS
