"""The slice plan of the decode attention's key split across workgroups (ovqa_attention_decode_split), on the host.

The plan is pure arithmetic in the library: chunk = ceil(n / splits) rounded up to 64 keys, slices = ceil(n / chunk), slice s
= keys [s * chunk, min((s + 1) * chunk, n)).  These tests need the built library and no GPU: no kernel is launched.
"""
import os
import re

from openvivqa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ovqa_attention_decode_split", "ovqa_attention_decode_split_slices",
         "ovqa_attention_decode_split_workspace_bytes", "ovqa_attention_decode_auto_splits"]


def plan(n, splits):
    """The documented plan, computed here: (chunk, [(lo, hi), ...])."""
    chunk = (-(-n // splits) + 63) // 64 * 64
    return chunk, [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]


def test_slices_tile_the_keys():
    lib = _lib.load()
    for n in range(1, 4101):
        for splits in range(1, 33):
            s_eff = lib.ovqa_attention_decode_split_slices(n, splits)
            chunk, slices = plan(n, splits)
            assert s_eff == len(slices), (n, splits, s_eff, len(slices))
            assert 1 <= s_eff <= splits, (n, splits, s_eff)
            if n <= 64 or splits == 1:
                assert s_eff == 1, (n, splits, s_eff)
            # the slices tile [0, n) exactly, none is empty, every start is a multiple of 64
            at = 0
            for s in range(s_eff):
                lo, hi = s * chunk, min((s + 1) * chunk, n)
                assert lo == at and hi > lo and lo % 64 == 0, (n, splits, s, lo, hi)
                at = hi
            assert at == n, (n, splits, at)


def test_slices_refuse_what_is_out_of_range():
    lib = _lib.load()
    for n, splits in ((0, 4), (-1, 4), (100, 0), (100, 33), (100, -2), ((1 << 30) + 1, 2)):
        assert lib.ovqa_attention_decode_split_slices(n, splits) == -1, (n, splits)
    assert lib.ovqa_attention_decode_split_slices(1 << 30, 32) == 32


def test_workspace_bytes():
    lib = _lib.load()
    for R, H, n, d in ((1, 8, 617, 64), (3, 3, 65, 32), (24, 8, 2049, 128), (1, 1, 1, 32), (5, 2, 4100, 64)):
        last = 0
        for splits in range(1, 33):
            b = lib.ovqa_attention_decode_split_workspace_bytes(R, H, n, d, splits)
            s_eff = lib.ovqa_attention_decode_split_slices(n, splits)
            assert b > 0 and b % 16 == 0, (R, H, n, d, splits, b)
            assert b >= R * H * s_eff * (d + 2) * 4  # a (maximum, sum, o[d]) fp32 record per (row, head, slice)
            assert b >= last, (R, H, n, d, splits, b, last)  # monotone in splits
            last = b
        # splits = 0 (the automatic rule): enough for whatever it picks
        assert lib.ovqa_attention_decode_split_workspace_bytes(R, H, n, d, 0) == last


def test_the_four_entries_are_declared():
    hdr = open(os.path.join(ROOT, "include", "ovqa_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 12 and _lib.load().ovqa_abi_version() == 12
    assert re.search(r"#define\s+OVQA_ABI_VERSION\s+12\b", hdr)


def test_python_wrappers():
    from openvivqa_amd import ops
    assert ops.decode_split_slices(2049, 8) == 7 and ops.decode_split_slices(40, 4) == 1
    assert ops.decode_split_workspace_bytes(1, 8, 2049, 64, 8) == 8 * 7 * 66 * 4


def test_too_many_keys_is_refused_as_by_the_unsplit_entry():
    """n > 2^30: OVQA_ERR_UNSUPPORTED (-2) from both entries, before any pointer is read or anything is launched."""
    lib = _lib.load()
    n, p = (1 << 30) + 1, 4096  # (p: a non-NULL, 16-byte aligned address that is never dereferenced)
    common = (1, p, 128, p, 128, p, 128, 128 * n, 1, None, 0, p, 128, 1, 2, n, 64, 0.125)
    assert lib.ovqa_attention_decode(*common, None) == -2
    assert lib.ovqa_attention_decode_split(*common, 4, p, 1 << 20, None) == -2
    assert lib.ovqa_attention_decode_split(*common, 33, p, 1 << 20, None) == -1  # splits out of 0 .. 32: OVQA_ERR_BAD_ARG
