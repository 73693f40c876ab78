"""Addresses and vectors shared by the per-track OSC address tests (tests/test_osc_addresses_cpu.py, test_gpu_osc_addresses.py; the
C++ programs tests/cpp/osc_table_host.cpp and osc_routes_host.cpp build the same address set).  An address of n bytes pads to
(n + 4) & ~3: the lengths cover every residue mod 4, both ends (1 and FX_OSC_ADDRESS_MAX = 124) and the word boundaries around 4,
8, 16 and 64."""
import numpy as np

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 63, 64, 65, 123, 124]
_FILL = "Mixer/Drums/Kick_0123456789-ABCDEFGHIJKLMNOPQRSTUVWXYZ~!#"


def address(length, track=0):
    """'/' and length - 1 printable bytes that differ from track to track"""
    body = "".join(_FILL[(track * 7 + k) % len(_FILL)] for k in range(length - 1))
    return "/" + body


def addresses(n, offset=0):
    """track c gets length LENGTHS[(c + offset) % 14]: neighbouring tracks differ in length"""
    return [address(LENGTHS[(c + offset) % len(LENGTHS)], c) for c in range(n)]


def message_bytes(addr):
    return ((len(addr) + 4) & ~3) + 64


def vectors(n, seed=0):
    """[n][12] float32 with the values a message must carry unchanged: NaN (getValue before the first insert), +-inf, -0.0"""
    v = np.random.default_rng(seed).standard_normal((n, 12)).astype(np.float32)
    v[0, 5] = np.inf
    v[n // 2, 2] = np.nan
    v[-1, 8] = -np.inf
    v[-1, 0] = -0.0
    return v
