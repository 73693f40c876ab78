"""The channel-list contract (csrc/fx_context.h, fx_check_channel_list / fx_check_channel_entries) is ONE contract: every entry of
include/fx.h that takes a list of tracks refuses a negative count, a null list with entries and an entry out of range with the same
words, before any device use -- and the setters that bring values of their own judge those between the list and the range of its
entries.  No GPU: a zeroed block stands in for a context (no tracks, no unit attached), and one whose track count is 1 for the rows
that need a good entry before the bad one."""
import ctypes
import struct

import pytest

ints = lambda *v: (ctypes.c_int * len(v))(*v)                          # noqa: E731
floats = lambda *v: (ctypes.c_float * len(v))(*v)                      # noqa: E731
BUF = (ctypes.c_float * 64)()
HOST, SELF, STOP = 0, 0, 2                                             # FX_MEM_HOST, FX_LISTEN_SELF, FX_STOP

# name -> the arguments behind (context, channels, num_channels), good ones for a list of two entries
ENTRIES = {
    "fx_reset_channels": (),
    "fx_clear_pending_channels": (),
    "fx_export_channels": (BUF, ctypes.sizeof(BUF), HOST),
    "fx_import_channels": (BUF, ctypes.sizeof(BUF), HOST),
    "fx_set_channel_clips": (ints(-1, -1), None),
    "fx_set_channel_sources": (ints(0, 0),),
    "fx_transport": (STOP,),
    "fx_set_channel_monitor": (None, None, None),
    "fx_set_channel_listen": (ints(SELF, SELF),),
    "fx_clear_display_channels": (),
    "fx_get_display": (BUF, HOST),
}
# the setters' own values: a bad one at entry 0 beside a bad channel at entry 0 -> what the call says
OWN_VALUES = {
    "fx_set_channel_clips": ((ints(3), None), b"entry 0: unknown clip id 3"),
    "fx_set_channel_sources": ((ints(2),), b"entry 0: unknown source 2"),
    "fx_transport": ((99,), b"unknown transport command 99"),
    "fx_set_channel_monitor": ((None, floats(float("inf")), None), b"entry 0: the left gain inf is not a finite number"),
    "fx_set_channel_listen": ((ints(7),), b"entry 0: unknown listen 7"),
}


def stand_in(tracks=0):
    """a zeroed context; fx_context begins {int device; int C; ...} -- if that moves, the range message below shows another C"""
    block = ctypes.create_string_buffer(1 << 16)
    struct.pack_into("i", block, 4, tracks)
    return block


def test_the_table_is_the_eleven_list_taking_entries(fx):
    assert len(ENTRIES) == 11 and set(OWN_VALUES) <= set(ENTRIES)
    for name in ENTRIES:
        assert name in fx.capi.EXPORTS, name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_entry_refuses_a_bad_list_with_the_same_words(fx, name):
    lib = fx.load_library()
    call, rest = getattr(lib, name), ENTRIES[name]
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    none, one = stand_in(0), stand_in(1)
    for ctx, channels, n, says in [
            (None, ints(0, 0), 2, b"null context"),
            (none, ints(0, 0), -1, b"negative channel count -1"),
            (none, None, 2, b"null channel list with 2 entries"),
            (one, ints(0, 1), 2, b"entry 1: channel 1 out of range [0,1)"),
            (one, ints(0, -3), 2, b"entry 1: channel -3 out of range [0,1)"),
            (none, ints(0, 0), 2, b"entry 0: channel 0 out of range [0,0)")]:
        assert call(ctx, channels, n, *rest) == INVALID, (name, says)
        assert lib.fx_last_error() == says, (name, lib.fx_last_error(), says)


@pytest.mark.parametrize("name", sorted(OWN_VALUES))
def test_a_setters_own_values_come_before_the_range_of_its_entries(fx, name):
    lib = fx.load_library()
    rest, says = OWN_VALUES[name]
    none = stand_in(0)
    assert getattr(lib, name)(none, ints(0), 1, *rest) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert lib.fx_last_error() == says, (name, lib.fx_last_error())
    # and behind the list's own refusals
    assert getattr(lib, name)(none, None, 1, *rest) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert lib.fx_last_error() == b"null channel list with 1 entries", (name, lib.fx_last_error())
