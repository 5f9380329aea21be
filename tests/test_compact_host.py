"""Compacting a live corpus, host side (include/gdr_hip_compact.h): the exported symbols and their prototypes, the
workspace sizing and every pre-launch refusal of the four calls, and the numpy restatement on hand-made cases.  Needs no GPU: the
pointers handed to the library are fakes that are never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

import compact_ref
from conftest import REPO
from gdr_amd import _ffi

CTYPE = {"size_t": C.c_size_t, "int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
NAMES = {"gdr_rows_compact_plan_workspace_bytes", "gdr_rows_compact_plan", "gdr_rows_compact_workspace_bytes", "gdr_rows_compact",
         "gdr_ids_remap", "gdr_rowmask_compact"}
EINVAL, ENOSPC = _ffi.GDR_EINVAL, _ffi.GDR_ENOSPC
BOUNCE = 64 << 20


def _strip(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _header():
    text = _strip(open(os.path.join(REPO, "include", "gdr_hip_compact.h")).read())
    return {m.group(2): (m.group(1), " ".join(m.group(3).split()))
            for m in re.finditer(r"\b(size_t|int)\s+(gdr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_exported_and_the_header_prototypes_match_the_binding():
    protos = _header()
    assert set(protos) == set(_ffi.COMPACT_SIGNATURES) == NAMES
    assert not set(_ffi.COMPACT_SIGNATURES) & (set(_ffi.SIGNATURES) | set(_ffi.PREFILTER_MASK_SIGNATURES))
    l = _ffi.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(l, name)                                                  # AttributeError: the library does not export it
        res, args = _ffi.COMPACT_SIGNATURES[name]
        assert fn.restype is res is CTYPE[ret] and fn.argtypes == args
        want = [C.c_void_p if "*" in p else CTYPE[p.split()[-2]] for p in params.split(",")]
        assert args == want, (name, params)
    assert l.gdr_abi_version() == 9 == _ffi.ABI_VERSION


def test_the_main_header_includes_the_new_one_and_declares_none_of_it():
    import test_abi_memory_host as main_host
    main = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert '#include "gdr_hip_compact.h"' in main, "gdr_hip.h must declare the whole ABI"
    code = re.sub(r"//[^\n]*", " ", _strip(main))
    for name in NAMES:
        assert name not in code, f"{name} appears in gdr_hip.h outside a comment"
    assert set(main_host._prototypes()) == set(_ffi.SIGNATURES)                # gdr_hip.h's own symbol set is what it was
    text = open(os.path.join(REPO, "include", "gdr_hip_compact.h")).read()
    assert int(re.search(r"#define GDR_COMPACT_BOUNCE_BYTES (\d+)", text).group(1)) == BOUNCE
    flat = " ".join(text.replace("*", " ").split())
    for phrase in ("No float atomics", "can never overlap a LATER chunk's sources", "neither read nor written", "GDR_ENOSPC before any launch",
                   "nothing is then written past out_old_id[n_live)", "does not depend on N"):
        assert phrase in flat, phrase


def test_workspace_sizes_are_monotone():
    l = _ffi.lib()
    plan = l.gdr_rows_compact_plan_workspace_bytes
    ns = [1, 31, 32, 33, 4095, 4096, 4097, 20_011, 320_000, 4096 * 1024 - 1, 4096 * 1024, 4096 * 1024 + 1, 10 ** 8, 2 ** 31 - 1]
    sizes = [plan(n) for n in ns]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] == 4 * 2 ** 19 and plan(4096) == 256 and plan(64 * 4096 + 1) == 512    # one int32 per tile of 4096 rows
    assert plan(0) == 0 and plan(-5) == 0 and plan(2 ** 31) == 0
    rows = l.gdr_rows_compact_workspace_bytes
    rbs = [4, 12, 192, 200, 256, 1536, 3072, 4096, BOUNCE - 4, BOUNCE, BOUNCE + 4, 1 << 30]
    for chunk in (0, 1, 64, 4096, 10 ** 6):
        got = [rows(rb, chunk) for rb in rbs]
        assert all(a <= b for a, b in zip(got, got[1:])), (chunk, got)
        if chunk:
            assert got == [chunk * rb + 256 for rb in rbs]
    for rb in rbs:
        got = [rows(rb, c) for c in (1, 2, 63, 64, 65, 4096, 10 ** 6)]
        assert all(a < b for a, b in zip(got, got[1:])), (rb, got)
        assert rows(rb, 0) == max(BOUNCE, rb) + 256                            # the default: a fixed size, whatever N is
        assert rows(rb, 0) >= rows(rb, max(BOUNCE // rb, 1))
    assert rows(0, 4) == 0 and rows(-4, 4) == 0 and rows(4, -1) == 0


def test_every_refusal_comes_before_any_launch_and_names_the_argument():
    l = _ffi.lib()
    p, q, ws = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 34)
    n0 = l.gdr_launch_count()
    err = lambda: l.gdr_last_error()   # noqa: E731
    N, n_live, rb = 1000, 600, 256

    plan = lambda N=N, n_live=n_live, words=p, new=q, old=q, st=q, w=ws, nbytes=1 << 20: l.gdr_rows_compact_plan(words, N, n_live, new, old, st, w, nbytes, None)   # noqa: E731
    assert plan(N=0) == EINVAL and b"N=0" in err()
    assert plan(N=2 ** 31) == EINVAL and b"N=" in err()
    assert plan(n_live=N + 1) == EINVAL and b"n_live=1001" in err()
    assert plan(n_live=-1) == EINVAL and b"n_live" in err()
    assert plan(words=None) == EINVAL and b"null" in err()
    assert plan(old=None) == EINVAL and b"out_old_id" in err()
    assert plan(st=None) == EINVAL and plan(w=None) == EINVAL
    need = l.gdr_rows_compact_plan_workspace_bytes(N)
    assert plan(nbytes=need - 1) == ENOSPC and str(need).encode() in err() and str(need - 1).encode() in err()

    rows = lambda src=p, dst=q, N=N, rb=rb, old=p, n_live=n_live, chunk=0, w=ws, nbytes=1 << 40: l.gdr_rows_compact(src, dst, N, rb, old, n_live, chunk, w, nbytes, None)   # noqa: E731
    for bad in (0, 2, 6, -4):
        assert rows(rb=bad) == EINVAL and f"row_bytes={bad}".encode() in err(), bad
        assert rows(dst=p, rb=bad) == EINVAL
    assert rows(n_live=N + 1) == EINVAL and b"n_live=1001" in err()
    assert rows(N=0, n_live=0) == EINVAL and b"N=0" in err()
    assert rows(chunk=-1) == EINVAL and b"chunk_rows" in err()
    assert rows(src=None) == EINVAL and rows(old=None) == EINVAL and b"old_id" in err()
    assert rows(src=C.c_void_p((1 << 20) + 2), dst=C.c_void_p((1 << 20) + 2)) == EINVAL and b"aligned" in err()
    # a visible partial overlap: dst starts inside src's N rows, and src starts inside dst's n_live rows
    for src, dst in (((1 << 20), (1 << 20) + rb), ((1 << 20), (1 << 20) + (N - 1) * rb), ((1 << 20) + rb, (1 << 20)), ((1 << 20) + (n_live - 1) * rb, (1 << 20))):
        assert rows(src=C.c_void_p(src), dst=C.c_void_p(dst)) == EINVAL and b"dst overlaps src" in err(), (src, dst)
    # in place: a workspace one byte short of the declared size, for an explicit chunk and for the default; and none at all
    for chunk in (0, 1, 64, 4096):
        need = l.gdr_rows_compact_workspace_bytes(rb, chunk)
        assert rows(dst=p, chunk=chunk, nbytes=need - 1) == ENOSPC, chunk
        assert str(need).encode() in err() and str(need - 1).encode() in err()
    assert rows(dst=p, w=None, nbytes=0) == ENOSPC
    # what needs no launch answers GDR_OK: nothing live
    assert rows(n_live=0, w=None, nbytes=0) == 0
    assert rows(dst=p, n_live=0, nbytes=l.gdr_rows_compact_workspace_bytes(rb, 0)) == 0

    remap = lambda new=p, N=N, ids=q, out=q, n=10, st=ws: l.gdr_ids_remap(new, N, ids, out, n, st, None)   # noqa: E731
    assert remap(N=0) == EINVAL and b"N=0" in err()
    assert remap(n=-1) == EINVAL and b"n=-1" in err()
    assert remap(new=None) == EINVAL and remap(st=None) == EINVAL and b"out_status" in err()
    assert remap(ids=None) == EINVAL and remap(out=None) == EINVAL and b"out_ids" in err()
    assert remap(out=C.c_void_p((1 << 30) + 8)) == EINVAL and b"partly overlaps" in err()

    W, Wn = (N + 31) // 32, (n_live + 31) // 32
    mask = lambda win=p, si=W + 3, B=5, N=N, old=ws, n_live=n_live, wout=q, so=Wn + 1: l.gdr_rowmask_compact(win, si, B, N, old, n_live, wout, so, None)   # noqa: E731
    assert mask(N=0) == EINVAL and b"N=0" in err()
    assert mask(n_live=N + 1) == EINVAL and b"n_live" in err()
    assert mask(B=-1) == EINVAL and b"B=-1" in err()
    assert mask(si=W - 1) == EINVAL and b"in_stride_words" in err()
    assert mask(so=Wn - 1) == EINVAL and b"out_stride_words" in err()
    assert mask(win=None) == EINVAL and mask(wout=None) == EINVAL and mask(old=None) == EINVAL and b"null" in err()
    assert mask(wout=p) == EINVAL and b"must not alias" in err()
    assert mask(wout=C.c_void_p((1 << 20) + 4 * (W + 3) * 4)) == EINVAL and b"must not alias" in err()   # inside the last input bitmap
    assert mask(B=0) == 0 and mask(n_live=0, so=0) == 0
    assert l.gdr_launch_count() == n0


def test_the_restatement_on_hand_made_cases():
    live = np.array([0, 1, 1, 0, 0, 1, 0, 1, 1], bool)
    new_id, old_id = compact_ref.plan(live)
    assert new_id.tolist() == [-1, 0, 1, -1, -1, 2, -1, 3, 4] and old_id.tolist() == [1, 2, 5, 7, 8]
    assert compact_ref.pack(live).tolist() == [0b110100110] and compact_ref.unpack(compact_ref.pack(live), 9).tolist() == live.tolist()
    assert compact_ref.pack(np.ones(33, bool)).view(np.uint32).tolist() == [0xFFFFFFFF, 1]
    T = np.arange(18).reshape(9, 2)
    assert compact_ref.rows(T, old_id).tolist() == [[2, 3], [4, 5], [10, 11], [14, 15], [16, 17]]
    assert compact_ref.rows_in_place(T, old_id)[5:].tolist() == T[5:].tolist()
    out, st = compact_ref.remap(new_id, [-1, 1, 8, -7])
    assert out.tolist() == [-1, 0, 4, -7] and st == 0
    out, st = compact_ref.remap(new_id, [1, 0, 9, 2 ** 31 - 1])
    assert out.tolist() == [0, -1, -1, -1] and st == 1
    allowed = np.array([[1, 1, 0, 0, 1, 1, 0, 0, 1], [0, 0, 1, 0, 0, 0, 0, 1, 0]], bool)
    assert compact_ref.rowmask(allowed, old_id).tolist() == [[0b10101], [0b01010]]
    assert compact_ref.index_members([8, 1, 5], new_id).tolist() == [4, 0, 2]
    second = np.array([1, 0, 1, 1, 0], bool)
    n2, o2 = compact_ref.plan(second)
    both = live.copy()
    both[old_id[~second]] = False
    assert np.array_equal(compact_ref.compose(new_id, n2), compact_ref.plan(both)[0])
