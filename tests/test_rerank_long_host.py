"""The host side of the long-list rerank (more than 8192 candidates per query; csrc/rerank.hip rerank_impl): the workspace
size and the argument checks, which come before any launch and before any pointer is dereferenced — no GPU needed."""
import ctypes as C

import pytest


def _ceil256(n):
    return -(-n // 256) * 256


def test_workspace_bytes_keeps_the_short_size_and_grows_monotonically():
    from gdr_amd import _ffi, ops
    l = _ffi.lib()
    for B in (1, 3, 64):
        for mc in (1, 128, 8192):
            assert l.gdr_rerank_workspace_bytes(B, mc) == _ceil256(B * mc * 4), (B, mc)
        assert l.gdr_rerank_workspace_bytes(B, 8193) > _ceil256(B * 8193 * 4), B
    for bad in ((0, 5), (5, 0), (-1, 100), (100, -1)):
        assert l.gdr_rerank_workspace_bytes(*bad) == 0, bad
    cands = sorted({1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 8194, 10_000, 12_288, 12_289, 32_768, 32_769, 40_000, 65_537,
                    200_000, (1 << 20) - 1, 1 << 20} | {ops.RERANK_CHUNK * n + e for n in (2, 8, 9, 64) for e in (-1, 0, 1)})
    assert cands[-1] == ops.RERANK_LONG_MAX_CAND
    Bs = [1, 2, 3, 7, 8, 64, 65, 512]
    size = [[l.gdr_rerank_workspace_bytes(B, mc) for mc in cands] for B in Bs]
    for r, row in enumerate(size):
        assert all(x <= y for x, y in zip(row, row[1:])), ("max_cand", Bs[r])
        assert all(x % 256 == 0 for x in row)
    for lo, hi in zip(size, size[1:]):
        assert all(x <= y for x, y in zip(lo, hi)), "B"
    # the long form's size covers the score scratch and at least the chunk pass's lists of 8 alphas at k = 1024
    mc = 40_000
    assert l.gdr_rerank_workspace_bytes(2, mc) >= _ceil256(2 * mc * 4) + 2 * 8 * -(-mc // ops.RERANK_CHUNK) * 1024 * 8


def _entry_points():
    from gdr_amd import _ffi
    l = _ffi.lib()
    return [("gdr_rerank_topk", l.gdr_rerank_topk), ("gdr_rerank_topk_bf16", l.gdr_rerank_topk_bf16)]


def _call(fn, max_cand, k, flags, nbytes, B=2, R=10, A=3, d=64):
    p, ws = C.c_void_p(256), C.c_void_p(4096)                      # never dereferenced: every call below is refused first
    return fn(p, p, d, p, p, p, B, R, p, A, k, 0, p, p, max_cand, 0, 0, 1000, flags, ws, nbytes, None)


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_rerank_refuses_bad_long_list_arguments_before_any_launch(which):
    from gdr_amd import _ffi, ops
    l = _ffi.lib()
    name, fn = _entry_points()[which]
    big = 1 << 40
    too_long = ops.RERANK_LONG_MAX_CAND + 1
    assert _call(fn, too_long, 10, 0, big) == _ffi.GDR_EINVAL, name
    msg = l.gdr_last_error()
    assert b"max_cand" in msg and str(too_long).encode() in msg and str(ops.RERANK_LONG_MAX_CAND).encode() in msg, msg
    assert _call(fn, 8193, 1025, 0, big) == _ffi.GDR_EINVAL, name
    msg = l.gdr_last_error()
    assert b"k=1025" in msg and b"1024" in msg, msg
    assert _call(fn, 100, 1025, _ffi.RERANK_CHUNKED, big) == _ffi.GDR_EINVAL, name      # the flag brings the k rule with it
    assert b"k=1025" in l.gdr_last_error()
    for flags in (4, 4 | _ffi.RERANK_POSITIONS | _ffi.RERANK_CHUNKED, 1 << 30):
        assert _call(fn, 100, 10, flags, big) == _ffi.GDR_EINVAL, (name, flags)
        assert b"unknown flags" in l.gdr_last_error()
    # GDR_RERANK_CHUNKED needs the partial lists besides the score scratch: the short form's size is not enough
    for mc in (100, 8192):
        short = l.gdr_rerank_workspace_bytes(2, mc)
        assert _call(fn, mc, 10, _ffi.RERANK_CHUNKED, short) == _ffi.GDR_ENOSPC, (name, mc)
        msg = l.gdr_last_error().decode()
        need = int(msg.rsplit("required", 1)[1])
        assert short < need <= l.gdr_rerank_workspace_bytes(2, ops.RERANK_MAX_CAND + 1), msg   # the header's sizing rule serves
    # and a long list with the short form's formula is refused the same way
    assert _call(fn, 8193, 10, 0, _ceil256(2 * 8193 * 4)) == _ffi.GDR_ENOSPC, name
    assert _call(fn, 8193, 10, 0, l.gdr_rerank_workspace_bytes(2, 8193) - 1) == _ffi.GDR_ENOSPC, name


def test_the_binding_s_constants_are_the_header_s_and_the_kernel_s():
    import os
    import re
    from gdr_amd import _ffi, ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = open(os.path.join(repo, "include", "gdr_hip.h")).read()
    assert int(re.search(r"#define GDR_RERANK_CHUNKED (\d+)", head).group(1)) == _ffi.RERANK_CHUNKED == 2
    src = open(os.path.join(repo, "gdr_amd", "csrc", "rerank.hip")).read()
    const = lambda n: eval(re.search(r"constexpr int %s = ([^;]+);" % n, src).group(1))       # noqa: E731
    assert const("RR_MAX_CAND") == ops.RERANK_MAX_CAND == 8192
    assert const("RR_LONG_MAX_CAND") == ops.RERANK_LONG_MAX_CAND == 1 << 20
    assert const("RR_LCH") == ops.RERANK_CHUNK and ops.RERANK_CHUNK & (ops.RERANK_CHUNK - 1) == 0 and ops.RERANK_CHUNK <= 8192
