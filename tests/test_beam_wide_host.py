"""The host side of the wide beam decode (up to 1024 beams, up to 2^17 candidates per query and step; csrc/beam.hip
check_beam_dims / beam_layout): the two workspace size functions and the argument checks, which come before any launch and
before any pointer is dereferenced — no GPU needed.  The switch GDR_DECODE_BEAM_CHUNKED is read once per process, so its
effect on the sizes is looked at in a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BEAMS, MAX_CAND, SORT_MAX, CHUNK = 1024, 1 << 17, 8192, 4096

# gdr_beam_search_table_workspace_bytes(B, R, max_length, V) of the commit before the chunked select, for shapes that stay in
# the one-sort form (R * (V+1) <= 8192): they must not move
ONE_SORT_TABLE = {(1, 2, 2, 1): 6912, (2, 100, 5, 30): 70656, (1, 100, 10, 30): 51200, (64, 10, 10, 30): 305152,
                  (3, 70, 7, 10): 68096, (5, 16, 5, 6): 23808, (2, 256, 4, 31): 158464, (1, 256, 32, 31): 281344,
                  (4, 264, 6, 30): 379392, (1, 128, 10, 63): 79616}
# gdr_t5_generate_workspace_bytes(w, B, L, R, max_length) of that commit for the decoder of _weights() below
ONE_SORT_GENERATE = {(1, 40, 100, 10): 146671616, (4, 16, 10, 10): 119659520, (64, 40, 10, 10): 423405568,
                     (2, 512, 30, 8): 139644160, (1, 12, 256, 10): 217325312, (1, 40, 264, 5): 184780288}


def _weights(V=30, max_out_len=10):
    from gdr_amd import _ffi
    fake = 0x7f0000000000                      # a non-null "device" pointer: the host code must never dereference it
    dl = (_ffi.GdrT5DecLayer * 2)()
    for ly in dl:
        for f, _t in ly._fields_:
            setattr(ly, f, fake)
    alr = (_ffi.GdrAdaptorLayer * 1)()
    for f, _t in alr[0]._fields_:
        setattr(alr[0], f, fake)
    dims = _ffi.GdrT5Dims(V * max_out_len + 2, 768, 64, 3072, 12, 2, 32, 128, 1e-6)
    w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 1, 8, 2048, 1e-5, fake, fake, fake, fake, dl, alr, fake, fake)
    w._keep = (dl, alr)
    return w


def test_one_sort_shapes_keep_their_workspace_sizes():
    from gdr_amd import _ffi
    l = _ffi.lib()
    for shape, want in ONE_SORT_TABLE.items():
        assert shape[1] * (shape[3] + 1) <= SORT_MAX
        assert l.gdr_beam_search_table_workspace_bytes(*shape) == want, shape
    w = _weights()
    for (B, L, R, ml), want in ONE_SORT_GENERATE.items():
        assert R * 31 <= SORT_MAX
        assert l.gdr_t5_generate_workspace_bytes(C.byref(w), B, L, R, ml) == want, (B, L, R, ml)


def test_workspace_sizes_accept_wide_beams_and_grow_monotonically():
    from gdr_amd import _ffi
    l = _ffi.lib()
    Rs = [2, 6, 100, 256, 257, 264, 265, 300, 512, 1023, 1024]
    Vs = [1, 6, 7, 30, 31, 32, 63, 64, 100, 127]
    Bs, mls = [1, 2, 5, 64], [2, 5, 10, 13]
    size = {}
    for B in Bs:
        for ml in mls:
            for R in Rs:
                for V in Vs:
                    if R * (V + 1) > MAX_CAND:
                        continue
                    n = size[(B, ml, R, V)] = l.gdr_beam_search_table_workspace_bytes(B, R, ml, V)
                    assert n > 0 and n % 256 == 0, (B, ml, R, V)
                    if R * (V + 1) > SORT_MAX:   # the chunked form: the normalisers and the chunk pass's partial lists at least
                        assert n >= B * R * 8 + B * -(-R * (V + 1) // CHUNK) * 2 * R * 8, (B, ml, R, V)
    assert (1, 10, 1024, 127) in size and (1, 10, 257, 127) in size and (1, 10, 300, 30) in size
    for (B, ml, R, V), n in size.items():
        for other in ((Bs, 0, B), (mls, 1, ml), (Rs, 2, R), (Vs, 3, V)):
            axis, pos, val = other
            i = axis.index(val)
            if i + 1 < len(axis):
                key = list((B, ml, R, V))
                key[pos] = axis[i + 1]
                if tuple(key) in size:
                    assert size[tuple(key)] >= n, ((B, ml, R, V), tuple(key))
    # the model's function: the same additions on top of its own buffers, in every argument
    w = _weights(V=63)
    prev = 0
    for R in Rs:
        n = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 40, R, 10)
        assert n > prev, R
        prev = n
    w30 = _weights()
    g = lambda B, L, R, ml: l.gdr_t5_generate_workspace_bytes(C.byref(w30), B, L, R, ml)   # noqa: E731
    assert g(1, 40, 300, 10) - g(1, 40, 264, 10) > (300 - 264) * 31 * 4          # crossing into the chunked form adds its lists
    assert g(2, 40, 300, 10) >= g(1, 40, 300, 10) and g(1, 41, 300, 10) >= g(1, 40, 300, 10) and g(1, 40, 300, 11) >= g(1, 40, 300, 10)
    assert g(1, 40, 1024, 10) > g(1, 40, 1023, 10) > g(1, 40, 300, 10)


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from gdr_amd import _ffi
l = _ffi.lib()
shapes = json.loads(sys.argv[2])
print("RESULT " + json.dumps([int(l.gdr_beam_search_table_workspace_bytes(*s)) for s in shapes]))
"""


def test_the_forced_chunked_form_is_in_the_workspace_sizes():
    shapes = [list(k) for k in ONE_SORT_TABLE] + [[1, 300, 10, 30], [2, 1024, 5, 63]]

    def run(**env):
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(shapes)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    off, on = run(GDR_DECODE_BEAM_CHUNKED="0"), run(GDR_DECODE_BEAM_CHUNKED="1")
    assert off[:len(ONE_SORT_TABLE)] == list(ONE_SORT_TABLE.values())
    for s, a, b in zip(shapes, off, on):
        B, R, ml, V = s
        if R * (V + 1) <= SORT_MAX:      # forced: the normalisers, one chunk's list and the merge's output list
            assert b >= a + B * R * 8 + B * 2 * R * 8, s
        else:                            # chunked anyway
            assert a == b, s


def _table_call(l, B, V, R, ml, nret, nbytes):
    p = C.c_void_p(256)                                            # never dereferenced: every call below is refused first
    return l.gdr_beam_search_table(p, B, V, R, ml, 0.8, nret, None, p, p, p, C.c_void_p(4096), nbytes, None)


def _generate_call(fn, w, B, L, R, ml, nret, nbytes):
    p = C.c_void_p(256)
    return fn(C.byref(w), p, p, B, L, R, ml, 0.8, nret, None, None, p, p, p, None, None, C.c_void_p(4096), nbytes, None)


def test_beam_search_refuses_out_of_range_beams_before_any_launch():
    from gdr_amd import _ffi
    l = _ffi.lib()
    big = 1 << 44
    assert _table_call(l, 1, 30, 1025, 5, 10, big) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert b"num_beams=1025" in msg and b"1024" in msg, msg
    assert _table_call(l, 1, 30, 1, 5, 1, big) == _ffi.GDR_EINVAL
    assert b"num_beams=1" in l.gdr_last_error()
    # 2^17 candidates per query: 1024 beams x 128 columns (V = 127) are the last shape in
    for R, V in ((1024, 128), (683, 191), (2, 65536), (1000, 131)):
        assert R * (V + 1) > MAX_CAND
        assert _table_call(l, 1, V, R, 3, 2, big) == _ffi.GDR_EINVAL, (R, V)
        msg = l.gdr_last_error()
        assert b"num_beams*(V+1)" in msg and str(R * (V + 1)).encode() in msg and str(MAX_CAND).encode() in msg, msg
    # (131073 = 3 x 43691 itself is only reachable past the beam limit; 683 x 192 = 131136 is the nearest shape within it)
    # accepted shapes get as far as the workspace check: ENOSPC names the size the size function returns
    for R, V, ml in ((257, 30, 5), (300, 30, 10), (1024, 127, 5), (1024, 30, 13), (512, 63, 32), (256, 40, 4)):
        need = l.gdr_beam_search_table_workspace_bytes(2, R, ml, V)
        assert _table_call(l, 2, V, R, ml, R, need - 1) == _ffi.GDR_ENOSPC, (R, V, ml)
        msg = l.gdr_last_error().decode()
        assert int(msg.rsplit("required", 1)[1]) == need, msg


def test_the_hypothesis_heap_must_fit_a_workgroup_s_lds():
    """A query's heap of num_beams + 1 hypotheses of max_length tokens and, at the end, its open beam rows live in one
    workgroup's LDS (160 KiB on gfx950): 1024 beams fit up to max_length = 13, 512 beams up to the largest max_length."""
    from gdr_amd import _ffi
    l = _ffi.lib()
    big = 1 << 44
    for R, ml, ok in ((1024, 10, True), (1024, 13, True), (1024, 14, False), (1024, 32, False), (768, 20, True), (768, 21, False),
                      (512, 32, True), (300, 32, True), (256, 32, True)):
        need = l.gdr_beam_search_table_workspace_bytes(1, R, ml, 6)
        rc = _table_call(l, 1, 6, R, ml, R, need - 1)
        if ok:
            assert rc == _ffi.GDR_ENOSPC, (R, ml)
        else:
            assert rc == _ffi.GDR_EINVAL, (R, ml)
            msg = l.gdr_last_error()
            assert b"num_beams=%d" % R in msg and b"max_length=%d" % ml in msg and b"LDS" in msg, msg


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_generate_takes_the_same_rules(which):
    from gdr_amd import _ffi
    l = _ffi.lib()
    fn = (l.gdr_t5_generate, l.gdr_t5_generate_bf16)[which]
    w, big = _weights(), 1 << 44
    assert _generate_call(fn, w, 2, 16, 1025, 10, 10, big) == _ffi.GDR_EINVAL
    assert b"num_beams=1025" in l.gdr_last_error()
    w127 = _weights(V=130, max_out_len=4)
    assert _generate_call(fn, w127, 2, 16, 1024, 4, 10, big) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert b"num_beams*(V+1)" in msg and str(1024 * 131).encode() in msg, msg
    w32 = _weights(V=6, max_out_len=32)
    assert _generate_call(fn, w32, 2, 16, 1024, 32, 10, big) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert b"num_beams=1024" in msg and b"max_length=32" in msg, msg
    for R in (257, 300, 1024):
        need = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, R, 10)
        assert _generate_call(fn, w, 2, 16, R, 10, R, need - 1) == _ffi.GDR_ENOSPC, R
        assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) == need


def test_the_beam_ceiling_is_the_rerank_s():
    import re
    src = lambda n: open(os.path.join(ROOT, "gdr_amd", "csrc", n)).read()          # noqa: E731
    assert int(re.search(r"constexpr int GDR_MAX_BEAMS = (\d+);", src("common.h")).group(1)) == MAX_BEAMS
    assert re.search(r"constexpr int RR_MAX_BEAMS = GDR_MAX_BEAMS;", src("rerank.hip"))
    assert re.search(r"bd\.R <= GDR_MAX_BEAMS", src("beam.hip"))
    head = open(os.path.join(ROOT, "include", "gdr_hip.h")).read()
    assert "2 <= num_beams <= 1024" in head and "131072" in head and "GDR_DECODE_BEAM_CHUNKED" in head
