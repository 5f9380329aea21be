"""The C ABI's memory contract (include/gdr_hip.h), entry point by entry point, as a foreign caller would meet it: the calls go
through _ffi.lib() with raw pointers.  Three properties that value tests on torch-allocated tensors cannot see:

  (a) NO WRITE outside an output or outside the declared workspace: every output sits in a guarded buffer (tests/abi_guard.py),
      the workspace is EXACTLY *_workspace_bytes(...) bytes and guarded; the bands are compared after every call; inputs
      are compared unchanged (except where the header lets an argument alias).
  (b) NO DEPENDENCE on what scratch held before the call: the same call with the workspace pre-filled with 0x00, 0xFF and
      0x5A gives bit-identical results, equal to what the gdr_amd.ops path returns for the same inputs; and
  (c) run twice on the same poisoned buffer without re-filling (warm state) it gives the same bits again.
  (d) One comparison with a plain float64 / oracle reference at the sibling test's tolerance: a guard test that passes on
      garbage proves nothing.
  Reads past the logical end of an input: the inputs sit in guarded buffers whose tail would change the answer if read — rows
  behind D that outscore every real row for every query (checked on the CPU) and large finite rows behind Q, NaN rows behind A / W / the residual, in-range ids of high-scoring documents behind
  candidate arrays, valid token ids behind token arrays.

The words a waiting workgroup spins on are the stream-K flags of gemm_f32.hip only (every other cross-workgroup hand-off of
the library is a last-arriver ticket, which never waits); they are zeroed by a memset on the call's stream in
gdr_linear_f32_splitk, in the T5 / BERT forwards and in generate before any launch that reads them (the prefix-table build
hands its linears no stream-K scratch and never takes that form), so a poisoned workspace documents a property the code claims; gdr_device_fault_pending() == 0 is asserted after every case.

COVERAGE (read by tests/test_abi_memory_host.py): entry point -> the tests of this file that hold it to (a)-(d)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from abi_guard import guarded, guarded_input, poisoned_workspace
from gdr_amd import _ffi, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = 1e-4                      # tests/test_gpu_parity.py: fp32 scores / logits abs(d) <= 1e-4 + 1e-4 * abs(ref)
FILLS = (0x00, 0xFF, 0x5A)
NAN = float("nan")

COVERAGE = {}
# entry points a test reaches through a gdr_amd.ops object (on guarded buffers the test hands it) instead of a direct call
VIA_OPS = {"gdr_t5_prefix_table_build": "PrefixTable", "gdr_t5_prefix_table_build_bf16": "PrefixTable"}


def covers(*names):
    def deco(fn):
        for n in names:
            COVERAGE.setdefault(n, []).append(fn.__name__)
        return fn
    return deco


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def same_bits(a, b):
    """Bit-for-bit equality of two tensors (NaN payloads and signed zeros included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def run_guarded(dev, out_specs, ws_bytes, call, inputs=(), init=None, cols=None, fills=FILLS, what="", project=None):
    """Properties (a), (b), (c) for one call.
    out_specs: {name: (shape, dtype)} — every output is allocated guarded, afresh for every fill;
    ws_bytes:  the exact workspace size (0: the call gets a NULL workspace);
    call(outs, ws, ws_bytes) -> rc: the raw ABI call (ws is a uint8 tensor or None);
    inputs:    guard handles of the inputs (guarded_input) — compared unchanged after all runs;
    init:      {name: tensor} copied into an output before every call (operands the header lets alias an output);
    cols:      {name: n} for a 2-D output [rows, ld] of which only [:, :n] may be written: the pad columns are compared with the
               guard pattern and the result is the [:, :n] block.
    project:   maps the outputs of a run to the part the contract defines (default: all of it).
    Returns {name: tensor} of the first run; all runs were bit-identical."""
    runs = []
    for fill in fills:
        outs, hs = {}, {}
        for name, (shape, dtype) in out_specs.items():
            outs[name], hs[name] = guarded(shape, dtype, dev)
        ws, wh = poisoned_workspace(ws_bytes, fill, dev)
        for rep in range(2 if fill == fills[-1] else 1):            # the last fill runs twice: warm scratch, not re-filled
            for name, t in (init or {}).items():
                n = (cols or {}).get(name)
                (outs[name] if n is None else outs[name][:, :n]).copy_(t)
            rc = call(outs, ws, ws_bytes)
            assert rc == 0, f"{what}: rc {rc}: {lib().gdr_last_error().decode()}"
            torch.cuda.synchronize()
            tag = f"{what} fill 0x{fill:02X}{' (warm)' if rep else ''}"
            for name, h in hs.items():
                h.check(f"{tag}: output {name}")
                if cols and name in cols:
                    h.check_columns(cols[name], f"{tag}: output {name}")
            if wh is not None:
                wh.check(f"{tag}: workspace of {ws_bytes} bytes")
            got = {name: (t if not (cols and name in cols) else t[:, :cols[name]]).clone() for name, t in outs.items()}
            runs.append((tag, project(got) if project else got))
    for h in inputs:
        h.unchanged(f"{what}: an input")
    assert lib().gdr_device_fault_pending() == 0, f"{what}: {lib().gdr_last_error().decode()}"
    tag0, first = runs[0]
    for tag, r in runs[1:]:
        for name in first:
            assert same_bits(first[name], r[name]), f"{what}: output {name} differs between [{tag0}] and [{tag}]"
    return first


# ================================================================================================ the helper tests itself
def test_guard_bands_catch_a_write_one_element_past_each_end(dev):
    for dtype in (torch.float32, torch.int32, torch.bfloat16):
        v, h = guarded((7, 12), dtype, dev)
        assert v.data_ptr() % 256 == 0 and h.lo >= 64 << 10 and h.flat.numel() - h.lo - h.nbytes >= 1 << 20
        h.check()
        v.fill_(3)                                                   # the whole logical region may be written
        h.check()
        esz = v.element_size()
        flat = h.flat
        keep = flat.clone()
        flat[h.lo + h.nbytes:h.lo + h.nbytes + esz].view(dtype).fill_(5)   # one element past the end
        with pytest.raises(AssertionError, match="after"):
            h.check()
        flat.copy_(keep)
        h.check()
        flat[h.lo - esz:h.lo].view(dtype).fill_(5)                      # one element before the start
        with pytest.raises(AssertionError, match="before"):
            h.check()
        flat.copy_(keep)
        flat[-1] = 0                                                    # the very last byte of the band
        with pytest.raises(AssertionError, match="after"):
            h.check()
        flat.copy_(keep)
        flat[0] = 0
        with pytest.raises(AssertionError, match="before"):
            h.check()
    # band sizes are conditions: 256 rows of a wide tensor
    v, h = guarded((3, 4096), torch.float32, dev)
    assert h.flat.numel() - h.lo - h.nbytes >= 256 * 4096 * 4
    # pad columns of a strided output
    v, h = guarded((5, 12), torch.float32, dev)
    v[:, :8] = 1.0
    h.check_columns(8)
    v[4, 8] = 1.0
    with pytest.raises(AssertionError, match="pad columns"):
        h.check_columns(8)
    # inputs: the tail follows the last element directly; any write is seen
    x = torch.arange(10, dtype=torch.float32)
    xv, xh = guarded_input(x, tail=torch.full((4,), 9.0))
    assert torch.equal(xv.cpu(), x) and xv.data_ptr() % 256 == 0
    assert torch.equal(xh.flat[xh.lo + 40:xh.lo + 56].view(torch.float32).cpu(), torch.full((4,), 9.0))
    xh.unchanged()
    xv[9] = 0.0
    with pytest.raises(AssertionError, match="modified"):
        xh.unchanged()
    # the exact-size workspace: the band starts at byte nbytes
    ws, wh = poisoned_workspace(1000, 0x5A, dev)
    assert ws.numel() == 1000 and bool((ws == 0x5A).all()) and ws.data_ptr() % 256 == 0
    wh.check()
    wh.flat[wh.lo + 1000] = 0x5A
    with pytest.raises(AssertionError, match=r"first at \+0"):
        wh.check()
    assert poisoned_workspace(0, 0, dev) == (None, None)


# ================================================================================================ linear family
EPIS = {"none": _ffi.EPI_NONE, "residual": _ffi.EPI_RESIDUAL, "relu": _ffi.EPI_RELU, "bias": _ffi.EPI_BIAS,
        "bias_relu": _ffi.EPI_BIAS_RELU, "bias_residual": _ffi.EPI_BIAS_RESIDUAL, "bias_gelu": _ffi.EPI_BIAS_GELU}


@functools.lru_cache(maxsize=4)
def _linear_data(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    return a, w, b, r


def _epilogue_ref(base, epi, b, r):
    """float64 epilogue over a float64 product."""
    x = base.clone()
    if epi in (_ffi.EPI_BIAS, _ffi.EPI_BIAS_RELU, _ffi.EPI_BIAS_RESIDUAL, _ffi.EPI_BIAS_GELU):
        x += b.double()
    if epi in (_ffi.EPI_RESIDUAL, _ffi.EPI_BIAS_RESIDUAL):
        x += r.double()
    if epi in (_ffi.EPI_RELU, _ffi.EPI_BIAS_RELU):
        x = torch.relu(x)
    if epi == _ffi.EPI_BIAS_GELU:
        x = torch.nn.functional.gelu(x)
    return x


def _padded(t, ld, fill=NAN):
    """[rows, k] -> [rows, ld] with `fill` in the pad columns."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _operand(t, ld, tail_rows=64):
    """An A / W / residual operand as the ABI sees it: rows of ld elements (pad columns NaN) in a guarded buffer, NaN rows behind
    the last one.  Returns (device view [rows, ld], handle)."""
    t = t.cpu()
    p = _padded(t, ld) if ld != t.shape[1] else t.contiguous()
    return guarded_input(p, tail=torch.full((tail_rows, ld), NAN, dtype=t.dtype))


def _linear_case(dev, kind, M, N, K, epi_name, pad=0, ws_bytes=0, inplace=False, terms=6, seed=None, value_rows=None):
    """One linear call under (a)-(c) + the NaN tails; returns (result [M,N] on the device, float64 reference or None).
    kind: f32 (gdr_linear_f32), splitk (gdr_linear_f32_splitk with exactly ws_bytes), bf16 (gdr_linear_bf16), split
    (gdr_linear_split_bf16 with `terms`).  pad > 0: lda = K' + pad, ldw = K' + 2 pad, ldc = N + pad, ldr = N + 3 pad (K' = the
    operand row: K, or the plane row of the split forms), NaN in the pad columns of A, W and the residual."""
    epi = EPIS[epi_name]
    a, w, b, r = _linear_data(M, N, K, seed if seed is not None else M * 7 + N * 3 + K)
    needs_b = epi in (_ffi.EPI_BIAS, _ffi.EPI_BIAS_RELU, _ffi.EPI_BIAS_RESIDUAL, _ffi.EPI_BIAS_GELU)
    needs_r = epi in (_ffi.EPI_RESIDUAL, _ffi.EPI_BIAS_RESIDUAL)
    if kind in ("f32", "splitk"):
        a_op, w_op = a, w
    elif kind == "bf16":
        a_op, w_op = a.bfloat16(), w.bfloat16()
    else:                                                            # plane rows made by the library itself, exactly 3 K / 2 K wide
        mk = (lambda x: ops.split_f16x2(x.to(dev))[:, :2 * K]) if terms == 2 else (lambda x: ops.split_bf16x3(x.to(dev), padded=False))
        a_op, w_op = mk(a).cpu().contiguous(), mk(w).cpu().contiguous()
    kp = a_op.shape[1]
    lda, ldw, ldc, ldr = kp + pad, kp + 2 * pad, N + pad, N + 3 * pad
    Ad, ah = _operand(a_op, lda)
    Wd, wh = _operand(w_op, ldw)
    handles = [ah, wh]
    Bd = Rd = None
    if needs_b:
        Bd, bh = guarded_input(b, tail=torch.full((256,), NAN))
        handles.append(bh)
    init = None
    if needs_r and inplace:
        ldr = ldc                                                    # the residual IS the output
        init = {"C": r.to(dev)}
    elif needs_r:
        Rd, rh = _operand(r, ldr)
        handles.append(rh)

    def call(outs, ws, nbytes):
        Cv = outs["C"]
        res = Cv if (needs_r and inplace) else Rd
        if kind == "f32":
            return lib().gdr_linear_f32(ptr(Ad), lda, ptr(Wd), ldw, ptr(Cv), ldc, M, N, K, epi, ptr(Bd), ptr(res), ldr, stream_ptr())
        if kind == "splitk":
            return lib().gdr_linear_f32_splitk(ptr(Ad), lda, ptr(Wd), ldw, ptr(Cv), ldc, M, N, K, epi, ptr(Bd), ptr(res), ldr, ptr(ws),
                                               nbytes, stream_ptr())
        if kind == "bf16":
            return lib().gdr_linear_bf16(ptr(Ad), lda, ptr(Wd), ldw, ptr(Cv), ldc, M, N, K, epi, ptr(Bd), ptr(res), ldr, stream_ptr())
        return lib().gdr_linear_split_bf16(ptr(Ad), lda, ptr(Wd), ldw, ptr(Cv), ldc, M, N, K, terms, epi, ptr(Bd), ptr(res), ldr,
                                           stream_ptr())

    what = f"{kind} linear {M}x{N}x{K} {epi_name}{' in place' if inplace else ''} pad {pad} ws {ws_bytes}"
    out = run_guarded(dev, {"C": ((M, ldc), torch.float32)}, ws_bytes if kind == "splitk" else 0, call, inputs=handles, init=init,
                      cols={"C": N}, what=what)["C"]
    assert not bool(torch.isnan(out).any()), f"{what}: NaN in the result — a pad column or a row behind an operand was read"
    ref = None
    if value_rows is not None:
        rows = value_rows
        if kind == "bf16":
            base = a_op[rows].double() @ w_op.double().T
        else:
            base = a[rows].double() @ w.double().T
        ref = _epilogue_ref(base, epi, b, r[rows])
    return out, ref


def _ops_linear(dev, kind, M, N, K, epi_name, ws_bytes=0, terms=6, seed=None):
    """The same product through gdr_amd.ops on plain torch tensors (dense operands)."""
    epi = EPIS[epi_name]
    a, w, b, r = _linear_data(M, N, K, seed if seed is not None else M * 7 + N * 3 + K)
    kw = {}
    if epi in (_ffi.EPI_BIAS, _ffi.EPI_BIAS_RELU, _ffi.EPI_BIAS_RESIDUAL, _ffi.EPI_BIAS_GELU):
        kw["bias"] = b.to(dev)
    if epi in (_ffi.EPI_RESIDUAL, _ffi.EPI_BIAS_RESIDUAL):
        kw["residual"] = r.to(dev)
    if kind == "f32":
        return ops.linear(a.to(dev), w.to(dev), epilogue=epi, **kw)
    if kind == "splitk":
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        if ws is None:
            return ops.linear(a.to(dev), w.to(dev), epilogue=epi, **kw)
        return ops.linear(a.to(dev), w.to(dev), epilogue=epi, splitk_ws=ws, **kw)
    if kind == "bf16":
        return ops.linear_bf16(a.to(dev), w.to(dev), epilogue=epi, **kw)
    if terms == 2:
        return ops.linear_split_bf16(ops.split_f16x2(a.to(dev)), ops.split_f16x2(w.to(dev)), K, epilogue=epi, terms=2, **kw)
    return ops.linear_split_bf16(ops.split_bf16x3(a.to(dev)), ops.split_bf16x3(w.to(dev)), K, epilogue=epi, terms=terms, **kw)


def _value_rows(M):
    return torch.unique(torch.cat([torch.arange(0, min(M, 40)), torch.arange(max(M - 140, 0), M)]))


STREAMK_BYTES = 33558528        # include/gdr_hip.h: 512 x 64 KiB + 4 KiB
# form -> (entry point kind, M, N, K, exact workspace bytes, the form gdr_linear_f32_form must report): ragged M and N in every form
# (128 x 128 tiles in gemm_f32.hip, 64 x 64 in gemm_small.hip).  The forms are the branches of launch_linear_f32_ws; the assertion
# in _f32_form keeps a later retune of the thresholds from moving a case to another kernel under the old name.
F32_FORMS = {
    "one_tile": ("f32", 100, 90, 36, 0, 1),                       # GDR_F32_FORM_TILES: 1 tile, K % 32 != 0
    "grid": ("f32", 1700, 1801, 64, 0, 1),                        # GDR_F32_FORM_TILES: 14 x 15 = 210 tiles
    "persistent": ("f32", 3000, 2901, 64, 0, 2),                  # GDR_F32_FORM_PERSISTENT: 24 x 23 = 552 tiles > 512
    "small": ("f32", 70, 201, 256, 0, 3),                         # GDR_F32_FORM_SMALL: gemm_small.hip, no scratch, no split
    "small_splitk": ("splitk", 70, 201, 1024, 1 << 20, 4),        # GDR_F32_FORM_SMALL_SPLITK: slabs + splitk_reduce_small_kernel
    "splitk_slabs": ("splitk", 1601, 130, 512, 48 << 20, 5),      # GDR_F32_FORM_SPLITK: M > 1536, the 128-row core split along K
    "streamk_mid": ("splitk", 2100, 2101, 64, STREAMK_BYTES, 6),  # GDR_F32_FORM_STREAMK_256: 17 x 17 = 289 tiles in (256, 512]
    "streamk_tail": ("splitk", 3000, 2901, 256, STREAMK_BYTES, 7),  # GDR_F32_FORM_STREAMK_TAIL: 552 tiles, 8 K-steps
}


def _f32_form(form):
    kind, M, N, K, wsb, want = F32_FORMS[form]
    got = lib().gdr_linear_f32_form(M, N, K, wsb)
    assert got == want, f"{form}: {M} x {N} x {K} with {wsb} bytes of scratch takes form {got}, the case was written for form {want}"
    return kind, M, N, K, wsb


@covers("gdr_linear_f32", "gdr_linear_f32_splitk", "gdr_linear_f32_form")
@pytest.mark.parametrize("form", list(F32_FORMS))
def test_linear_f32_forms_every_epilogue(dev, form):
    kind, M, N, K, wsb = _f32_form(form)
    rows = _value_rows(M)
    cases = [(e, False) for e in EPIS] + [("residual", True), ("bias_residual", True)]
    for epi_name, inplace in cases:
        out, ref = _linear_case(dev, kind, M, N, K, epi_name, ws_bytes=wsb, inplace=inplace, value_rows=rows)
        assert same_bits(out, _ops_linear(dev, kind, M, N, K, epi_name, ws_bytes=wsb)), f"{form} {epi_name}: differs from the ops path"
        torch.testing.assert_close(out[rows.to(dev)].cpu().double(), ref, rtol=TOL, atol=TOL, msg=f"{form} {epi_name}")


@covers("gdr_linear_f32_splitk")
@pytest.mark.parametrize("form", ["small_splitk", "splitk_slabs", "streamk_mid", "streamk_tail"])
@pytest.mark.parametrize("ws_bytes", [0, 1 << 20, STREAMK_BYTES, STREAMK_BYTES - 1, 48 << 20])
def test_linear_f32_splitk_adapts_to_the_workspace_it_is_given(dev, form, ws_bytes):
    """Any workspace size is legal: the launcher takes as many K slabs as fit (none: the whole-tile kernels), and the stream-K forms
    only from 33 558 528 bytes on — one byte less must not touch the flag words behind the hand-off scratch."""
    _, M, N, K, _ = _f32_form(form)
    # what each size must select: no scratch or too little for two slabs -> the whole-K kernels; stream-K only from STREAMK_BYTES on
    F = dict(TILES=1, PERSISTENT=2, SMALL=3, SMALL_SPLITK=4, SPLITK=5, STREAMK_256=6, STREAMK_TAIL=7)
    want = {"small_splitk": {0: F["SMALL"]}, "splitk_slabs": {0: F["TILES"], 1 << 20: F["TILES"]},
            "streamk_mid": {0: F["TILES"], 1 << 20: F["TILES"], STREAMK_BYTES - 1: F["TILES"]},
            "streamk_tail": {0: F["PERSISTENT"], 1 << 20: F["PERSISTENT"], STREAMK_BYTES - 1: F["PERSISTENT"]}}[form]
    assert lib().gdr_linear_f32_form(M, N, K, ws_bytes) == want.get(ws_bytes, F32_FORMS[form][5]), (form, ws_bytes)
    rows = _value_rows(M)
    for epi_name, inplace in (("none", False), ("bias_residual", True)):
        out, ref = _linear_case(dev, "splitk", M, N, K, epi_name, ws_bytes=ws_bytes, inplace=inplace, value_rows=rows)
        assert same_bits(out, _ops_linear(dev, "splitk", M, N, K, epi_name, ws_bytes=ws_bytes))
        torch.testing.assert_close(out[rows.to(dev)].cpu().double(), ref, rtol=TOL, atol=TOL)


@covers("gdr_linear_f32", "gdr_linear_f32_splitk")
@pytest.mark.parametrize("form", list(F32_FORMS))
def test_linear_f32_leading_dimensions(dev, form):
    """lda = K + pad, ldw = K + 2 pad, ldc = N + pad, ldr = N + 3 pad with pad = 4 (the smallest the header admits) and 12: NaN in the
    pad columns of A, W and the residual, the guard pattern in C's; C[:, :N] equals the dense call bit for bit (the same k-ordered
    chain per element) and C's pad columns are untouched."""
    kind, M, N, K, wsb = _f32_form(form)
    for epi_name in ("none", "bias_residual", "relu"):
        dense, _ = _linear_case(dev, kind, M, N, K, epi_name, ws_bytes=wsb)
        for pad in (4, 12):
            out, _ = _linear_case(dev, kind, M, N, K, epi_name, pad=pad, ws_bytes=wsb)
            assert same_bits(out, dense), f"{form} {epi_name} pad {pad}: strided result differs from the dense one"
    dense, _ = _linear_case(dev, kind, M, N, K, "residual", ws_bytes=wsb, inplace=True)
    out, _ = _linear_case(dev, kind, M, N, K, "residual", pad=4, ws_bytes=wsb, inplace=True)
    assert same_bits(out, dense)


# bf16: form -> (M, N, K, the tile form gdr_linear_bf16_tile_form must report).  Ragged M everywhere; ragged N where the form
# admits it (the 256-row tiles need N % 4 == 0).
BF16_FORMS = {
    "rows64": (333, 201, 128, 64),
    "rows128": (8200, 1153, 64, 128),          # 65 x 10 = 650 tiles >= 512
    "tile256x192": (8300, 2044, 2048, 192),
    "tile256x256": (8300, 1536, 2048, 256),
    "generic_core": (130, 129, 96, 0),
}


@covers("gdr_linear_bf16", "gdr_linear_bf16_tile_form")
@pytest.mark.parametrize("form", list(BF16_FORMS))
def test_linear_bf16_forms_epilogues_and_leading_dimensions(dev, form):
    M, N, K, want = BF16_FORMS[form]
    rows = _value_rows(M)
    for epi_name, inplace in (("none", False), ("bias_gelu", False), ("bias_residual", False), ("residual", True), ("relu", False)):
        assert lib().gdr_linear_bf16_tile_form(M, N, K, EPIS[epi_name]) == want, (form, epi_name)
        dense, ref = _linear_case(dev, "bf16", M, N, K, epi_name, inplace=inplace, value_rows=rows)
        assert same_bits(dense, _ops_linear(dev, "bf16", M, N, K, epi_name)), f"{form} {epi_name}: differs from the ops path"
        torch.testing.assert_close(dense[rows.to(dev)].cpu().double(), ref, rtol=TOL, atol=TOL, msg=f"{form} {epi_name}")
        if epi_name in ("none", "bias_residual", "residual"):
            for pad in (8, 24):                                      # bf16 operands: multiples of 8
                out, _ = _linear_case(dev, "bf16", M, N, K, epi_name, pad=pad, inplace=inplace)
                assert same_bits(out, dense), f"{form} {epi_name} pad {pad}: strided result differs from the dense one"


@covers("gdr_linear_split_bf16", "gdr_split_row_elems")
@pytest.mark.parametrize("terms,bound", [(6, 3e-5), (3, 1e-4), (2, 1.5e-5)])
@pytest.mark.parametrize("M,N,K", [(333, 201, 128), (8300, 768, 768)])
def test_linear_split_forms_and_leading_dimensions(dev, terms, bound, M, N, K):
    """The split linear on plane rows of exactly 3 K / 2 K elements and on padded ones (NaN pad); the error bound against float64
    is the sibling's (tests/test_gpu_parity.py: fraction of mean |c|)."""
    assert lib().gdr_split_row_elems(K, terms) == -(-(2 if terms == 2 else 3) * K // 64) * 64
    rows = _value_rows(M)
    prod, prod_ref = _linear_case(dev, "split", M, N, K, "none", terms=terms, value_rows=rows)   # the plain product, once
    for epi_name, inplace in (("none", False), ("bias_residual", False), ("residual", True)):
        dense, ref = (prod, prod_ref) if epi_name == "none" else \
            _linear_case(dev, "split", M, N, K, epi_name, terms=terms, inplace=inplace, value_rows=rows)
        got = dense[rows.to(dev)].cpu().double()
        if epi_name == "none":                                       # the sibling's two checks, unchanged: the product against float64 ...
            assert float((got - ref).abs().max()) <= bound * float(ref.abs().mean()), (terms, epi_name)
        else:                                                        # ... and an epilogue against the device's own product + bias + residual
            b_, r_ = _linear_data(M, N, K, M * 7 + N * 3 + K)[2:]
            want = prod[rows.to(dev)].cpu() + r_[rows] + (b_ if "bias" in epi_name else 0.0)
            torch.testing.assert_close(dense[rows.to(dev)].cpu(), want, rtol=1e-6, atol=1e-5)
        assert same_bits(dense, _ops_linear(dev, "split", M, N, K, epi_name, terms=terms))
        for pad in (8, 24):
            out, _ = _linear_case(dev, "split", M, N, K, epi_name, pad=pad, terms=terms, inplace=inplace)
            assert same_bits(out, dense), f"terms {terms} {epi_name} pad {pad}"


@covers("gdr_split_f32_bf16x3", "gdr_split_f32_f16x2", "gdr_cast_f32_bf16")
@pytest.mark.parametrize("rows,K", [(1, 4), (333, 68), (1000, 768)])
def test_split_and_cast_write_their_rows_only(dev, rows, K):
    g = torch.Generator().manual_seed(rows + K)
    x = torch.randn(rows, K, generator=g)
    xd, xh = guarded_input(x, tail=torch.full((64, K), NAN))
    for fn, planes, dtype, ops_fn in ((lib().gdr_split_f32_bf16x3, 3, torch.bfloat16, lambda t: ops.split_bf16x3(t, padded=False)),
                                      (lib().gdr_split_f32_f16x2, 2, torch.float16, None)):
        for ld in (planes * K, planes * K + 4, planes * K + 12):
            res = run_guarded(dev, {"out": ((rows, ld), dtype)}, 0,
                              lambda o, ws, n: fn(ptr(xd), ptr(o["out"]), rows, K, ld, stream_ptr()), inputs=[xh],
                              cols={"out": planes * K}, what=f"split planes {planes} ld {ld}")["out"].float().cpu()
            if planes == 3:
                hi = x.bfloat16()
                mid = (x - hi.float()).bfloat16()
                lo = (x - hi.float() - mid.float()).bfloat16()
                assert torch.equal(res, torch.cat([hi, mid, lo], 1).float())
                assert same_bits(res, ops_fn(x.to(dev)).float().cpu())
            else:
                hi = x.half()
                lo = ((x - hi.float()) * 2048.0).half()
                assert torch.equal(res, torch.cat([hi, lo], 1).float())
    res = run_guarded(dev, {"out": ((rows, K), torch.bfloat16)}, 0,
                      lambda o, ws, n: lib().gdr_cast_f32_bf16(ptr(xd), ptr(o["out"]), rows * K, stream_ptr()), inputs=[xh], what="cast")["out"]
    assert same_bits(res, ops.to_bf16(x.to(dev))) and torch.equal(res.cpu(), x.bfloat16())


# ================================================================================================ row-wise operators
@covers("gdr_t5_layer_norm", "gdr_l2_normalize")
@pytest.mark.parametrize("rows,d", [(1, 4), (7, 768), (259, 64), (1001, 1024)])
def test_row_norms_in_place_and_out_of_place(dev, rows, d):
    g = torch.Generator().manual_seed(rows * 3 + d)
    x, w = torch.randn(rows, d, generator=g) * 3.0, torch.randn(d, generator=g)
    xd, xh = guarded_input(x, tail=torch.full((64, d), NAN))
    wd, wh = guarded_input(w, tail=torch.full((256,), NAN))
    x64 = x.double()
    ln_ref = w.double() * (x64 / torch.sqrt((x64 * x64).mean(-1, keepdim=True) + 1e-6))
    l2_ref = x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    for name, fn, ref, ops_out in (
            ("t5_layer_norm", lambda src, dst: lib().gdr_t5_layer_norm(ptr(src), ptr(wd), ptr(dst), rows, d, 1e-6, stream_ptr()), ln_ref,
             ops.t5_layer_norm(x.to(dev), w.to(dev))),
            ("l2_normalize", lambda src, dst: lib().gdr_l2_normalize(ptr(src), ptr(dst), rows, d, 1e-12, stream_ptr()), l2_ref,
             ops.l2_normalize(x.to(dev)))):
        out = run_guarded(dev, {"y": ((rows, d), torch.float32)}, 0, lambda o, ws, n: fn(xd, o["y"]), inputs=[xh, wh], what=name)["y"]
        inp = run_guarded(dev, {"y": ((rows, d), torch.float32)}, 0, lambda o, ws, n: fn(o["y"], o["y"]), inputs=[wh], init={"y": x.to(dev)},
                          what=name + " in place")["y"]
        assert same_bits(out, inp) and same_bits(out, ops_out), name
        # fp32 against float64: a handful of roundings of 2^-24 each (sum of squares, sqrt, quotient, weight)
        torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-6, atol=1e-7, msg=name)


@covers("gdr_row_norm2_max")
@pytest.mark.parametrize("N,d", [(1, 4), (1003, 64), (70001, 128)])
def test_row_norm2_max_ignores_the_rows_behind_the_corpus(dev, N, d):
    D = synth.make_corpus(N, d, seed=N + d)
    Dd, dh = guarded_input(torch.from_numpy(D), tail=torch.full((256, d), 1e3))       # rows that would be the maximum if read
    out = run_guarded(dev, {"m": ((1,), torch.float32)}, 0, lambda o, ws, n: lib().gdr_row_norm2_max(ptr(Dd), N, d, ptr(o["m"]), stream_ptr()),
                      inputs=[dh], what="row_norm2_max")["m"]
    ref = float((D.astype(np.float64) ** 2).sum(1).max())
    assert abs(float(out[0]) - ref) <= 1e-5 * ref


# ================================================================================================ similarity + top-k
def _winning_rows(Q, D, n_rows, bf16=False):
    """n_rows rows that, placed behind D, would outscore every real document for EVERY query: the minimum-norm solution v of
    Q v = s 1 with s ten times the largest real score (the queries are linearly independent), scaled a little per row so
    that the rows differ.  Checked on the CPU, on the values the kernel would see."""
    Q64, D64 = Q.astype(np.float64), D.astype(np.float64)
    top = float(np.abs(Q64 @ D64.T).max())
    v = np.linalg.pinv(Q64) @ np.full(Q.shape[0], 10.0 * top + 1.0)
    tail = (v[None, :] * (1.0 + 0.01 * np.arange(n_rows)[:, None])).astype(np.float32)
    t = torch.from_numpy(tail)
    seen_t = t.bfloat16().float().numpy().astype(np.float64) if bf16 else tail.astype(np.float64)
    seen_q = torch.from_numpy(Q).bfloat16().float().numpy().astype(np.float64) if bf16 else Q64
    assert (seen_q @ seen_t.T).min() > 2.0 * top, "every tail row must take rank 1 for every query if admitted"
    return t


SIM_CASES = {
    # name: (B, N, d, k, flags, bf16)
    "f32_all_sample_gemm_k1": (5, 1000, 64, 1, 0, False),
    "f32_all_sample_gemm_k_eq_N": (5, 129, 32, 129, 0, False),
    "f32_sample_filter_gemm": (40, 40001, 64, 37, 0, False),
    "f32_sample_filter_gemm_k1024": (2, 20001, 64, 1024, 0, False),
    "f32_stream_sliced_tails": (8, 50001, 128, 37, 0, False),
    "f32_stream_all_sample_k_eq_N": (8, 1000, 128, 1000, 0, False),
    "f32_stream_k1024": (3, 30001, 256, 1024, 0, False),
    "f32_no_stream_flag": (8, 50001, 128, 37, _ffi.SIM_NO_STREAM, False),
    "f32_exhaustive_stream": (8, 50001, 128, 37, _ffi.SIM_EXHAUSTIVE, False),
    "f32_exhaustive_gemm": (40, 20001, 64, 10, _ffi.SIM_EXHAUSTIVE, False),
    "bf16_sample_filter_lds_dma": (40, 40001, 64, 37, 0, True),
    "bf16_all_sample_generic_core": (5, 3001, 40, 7, 0, True),
    "bf16_stream_sliced_tails": (8, 50001, 256, 37, 0, True),
    "bf16_no_stream_flag_k1": (8, 50001, 256, 1, _ffi.SIM_NO_STREAM, True),
    "bf16_exhaustive": (8, 20001, 256, 100, _ffi.SIM_EXHAUSTIVE, True),
}


@covers("gdr_sim_topk", "gdr_sim_topk_bf16")
@pytest.mark.parametrize("case", list(SIM_CASES))
def test_sim_topk_plans(dev, case):
    from conftest import order_insensitive_topk_match
    from oracle import retrieval_ref
    B, N, d, k, flags, bf16 = SIM_CASES[case]
    assert N % 128 != 0
    D = synth.make_corpus(N, d, seed=N + d)
    Q, _ = synth.make_queries(D, B, seed=B)
    # The last query points at the LAST document, so the row on the corpus's ragged edge is a rank-1 hit: kernels that clamp
    # the rows of the last tile to row N - 1 would, without their `row < N` mask, return copies of it under ids >= N.
    Q[B - 1] = D[N - 1]
    Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
    seen = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
    assert int((seen(Dt) @ seen(Qt[B - 1])).argmax()) == N - 1, "the last document must be the last query's best"
    d_tail = _winning_rows(Q, D, 256, bf16)
    q_tail = torch.full((128, d), 1e3)
    if bf16:
        Qt, Dt, d_tail, q_tail = Qt.bfloat16(), Dt.bfloat16(), d_tail.bfloat16(), q_tail.bfloat16()
    Qd, qh = guarded_input(Qt, tail=q_tail)
    Dd, dh = guarded_input(Dt, tail=d_tail)
    need = lib().gdr_sim_topk_workspace_bytes(B, N, d, k, flags)
    fn = lib().gdr_sim_topk_bf16 if bf16 else lib().gdr_sim_topk
    off = 1000
    res = run_guarded(dev, {"val": ((B, k), torch.float32), "idx": ((B, k), torch.int32), "status": ((B,), torch.int32)}, need,
                      lambda o, ws, n: fn(ptr(Qd), B, ptr(Dd), N, d, k, off, ptr(o["val"]), ptr(o["idx"]), ptr(o["status"]), flags, ptr(ws), n,
                                          stream_ptr()), inputs=[qh, dh], what=case)
    v, i, st = res["val"], res["idx"], res["status"]
    assert int(st.abs().sum()) == 0
    assert int(i.max()) < N + off and int(i.min()) >= off, "an id at or beyond N: a row behind the corpus was admitted"
    assert not bool(torch.isnan(v).any())
    ov, oi, ost = ops.sim_topk(Qt.to(dev), Dt.to(dev), k, idx_offset=off, return_status=True, exact_on_overflow=False, flags=flags)
    assert same_bits(v, ov) and same_bits(i, oi) and same_bits(st, ost), f"{case}: differs from the ops path on untailed tensors"
    rv, ri = retrieval_ref.sim_topk(Qt.float(), Dt.float(), k)
    order_insensitive_topk_match(rv.numpy(), ri.numpy(), v.cpu().numpy(), i.cpu().numpy().astype(np.int64) - off, TOL)
    assert (np.diff(v.cpu().numpy(), axis=1) <= 0).all()


@covers("gdr_sim_topk_prefilter")
@pytest.mark.parametrize("B,N,d,k", [(40, 40001, 128, 37), (8, 50001, 256, 100), (3, 1001, 64, 5)], ids=["gemm", "stream", "all_sample"])
def test_sim_topk_prefilter(dev, B, N, d, k):
    from conftest import order_insensitive_topk_match
    from oracle import retrieval_ref
    D = synth.make_corpus(N, d, seed=N + d)
    Q, _ = synth.make_queries(D, B, seed=B)
    Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
    tail = _winning_rows(Q, D, 256)
    _winning_rows(Q, D, 256, bf16=True)
    Qd, qh = guarded_input(Qt, tail=torch.full((128, d), 1e3))
    Dd, dh = guarded_input(Dt, tail=tail)
    D16, d16h = guarded_input(Dt.bfloat16(), tail=tail.bfloat16())
    P = ops.PrefilteredCorpus(Dt.to(dev))
    assert torch.equal(P.D16.cpu(), Dt.bfloat16())
    need = lib().gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k)
    res = run_guarded(dev, {"val": ((B, k), torch.float32), "idx": ((B, k), torch.int32), "status": ((B,), torch.int32)}, need,
                      lambda o, ws, n: lib().gdr_sim_topk_prefilter(ptr(Qd), B, ptr(Dd), ptr(D16), P.dnorm_max, N, d, k, 7, ptr(o["val"]),
                                                                    ptr(o["idx"]), ptr(o["status"]), ptr(ws), n, stream_ptr()),
                      inputs=[qh, dh, d16h], what="prefilter")
    v, i, st = res["val"], res["idx"], res["status"]
    assert int(st.abs().sum()) == 0 and int(i.max()) < N + 7 and int(i.min()) >= 7 and not bool(torch.isnan(v).any())
    ov, oi, ost = ops.sim_topk(Qt.to(dev), P, k, idx_offset=7, return_status=True, exact_on_overflow=False)
    assert same_bits(v, ov) and same_bits(i, oi) and same_bits(st, ost)
    rv, ri = retrieval_ref.sim_topk(Qt, Dt, k)
    order_insensitive_topk_match(rv.numpy(), ri.numpy(), v.cpu().numpy(), i.cpu().numpy().astype(np.int64) - 7, TOL)


def _total_order_key(v):
    """uint32 keys that sort fp32 values in IEEE total order (-0.0 below +0.0), the order include/gdr_hip.h states for scores."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))


def _merge_ref(vals, idx, k):
    """[G,B,k] -> [B,k]: higher score first (total order: +0.0 above -0.0), then lower id (numpy, stable)."""
    G, B, _ = vals.shape
    ov, oi = np.empty((B, k), np.float32), np.empty((B, k), np.int32)
    for b in range(B):
        v, i = vals[:, b].reshape(-1), idx[:, b].reshape(-1)
        order = np.lexsort((i, -_total_order_key(v).astype(np.int64)))[:k]
        ov[b], oi[b] = v[order], i[order]
    return ov, oi


@covers("gdr_topk_merge", "gdr_topk_pack", "gdr_topk_merge_packed")
@pytest.mark.parametrize("G,B,k", [(1, 1, 1), (4, 33, 50), (8, 5, 1024), (3, 130, 7)])
def test_topk_merge_pack_and_merge_packed(dev, G, B, k):
    rng = np.random.default_rng(G * 100 + B + k)
    vals = np.round(rng.standard_normal((G, B, k)).astype(np.float32), 1)          # rounded: many exact ties
    vals = -np.sort(-vals, axis=2)                                                 # rounding leaves -0.0 beside +0.0 among the ties
    for g in range(G):                                                              # a valid shard list: +0.0 in front of -0.0
        for b in range(B):
            vals[g, b] = vals[g, b][np.argsort(-_total_order_key(vals[g, b]).astype(np.int64), kind="stable")]
    idx = np.stack([np.sort(rng.choice(100000, size=(B, k), replace=False).astype(np.int32) % 12500 + g * 12500, axis=1)
                    for g in range(G)])
    status = (rng.random((G, B)) < 0.2).astype(np.int32)
    big = torch.full((B * k,), 1e30)
    Vd, vh = guarded_input(torch.from_numpy(vals), tail=big)                        # a shard behind the last one would win every slot
    Id, ih = guarded_input(torch.from_numpy(idx), tail=torch.arange(B * k, dtype=torch.int32))
    rv, ri = _merge_ref(vals, idx, k)
    res = run_guarded(dev, {"val": ((B, k), torch.float32), "idx": ((B, k), torch.int32)}, 0,
                      lambda o, ws, n: lib().gdr_topk_merge(ptr(Vd), ptr(Id), G, B, k, ptr(o["val"]), ptr(o["idx"]), stream_ptr()),
                      inputs=[vh, ih], what="topk_merge")
    ov, oi = ops.topk_merge(torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev))
    assert same_bits(res["val"], ov) and same_bits(res["idx"], oi)
    assert np.array_equal(res["val"].cpu().numpy().view(np.uint32), rv.view(np.uint32))       # bits: the sign of a zero counts
    assert np.array_equal(res["idx"].cpu().numpy(), ri)                             # ids exact: the tie rule is part of the contract
    # pack every shard, merge the packed rows
    packed = []
    for g in range(G):
        v1, v1h = guarded_input(torch.from_numpy(vals[g].copy()), tail=big[:k])
        i1, i1h = guarded_input(torch.from_numpy(idx[g].copy()), tail=torch.zeros(k, dtype=torch.int32))
        s1, s1h = guarded_input(torch.from_numpy(status[g].copy()), tail=torch.ones(256, dtype=torch.int32))
        p = run_guarded(dev, {"pairs": ((B, k + 1), torch.int64)}, 0,
                        lambda o, ws, n: lib().gdr_topk_pack(ptr(v1), ptr(i1), ptr(s1), B, k, ptr(o["pairs"]), stream_ptr()),
                        inputs=[v1h, i1h, s1h], what="topk_pack")["pairs"]
        assert same_bits(p, ops.topk_pack(torch.from_numpy(vals[g]).to(dev), torch.from_numpy(idx[g]).to(dev), torch.from_numpy(status[g]).to(dev)))
        pw = p.cpu().numpy().view(np.int32).reshape(B, k + 1, 2)
        assert np.array_equal(pw[:, :k, 0].view(np.float32), vals[g]) and np.array_equal(pw[:, :k, 1], idx[g])
        assert np.array_equal(pw[:, k, 1], status[g]) and not pw[:, k, 0].any()
        packed.append(p)
    tail_pair = torch.from_numpy(np.stack([np.full(B * (k + 1), 1e30, np.float32).view(np.int32), np.ones(B * (k + 1), np.int32)], 1)
                                 .reshape(-1).view(np.int64).copy())
    Pd, ph = guarded_input(torch.stack(packed).cpu(), tail=tail_pair)
    res2 = run_guarded(dev, {"val": ((B, k), torch.float32), "idx": ((B, k), torch.int32), "status": ((B,), torch.int32)}, 0,
                       lambda o, ws, n: lib().gdr_topk_merge_packed(ptr(Pd), G, B, k, ptr(o["val"]), ptr(o["idx"]), ptr(o["status"]),
                                                                    stream_ptr()), inputs=[ph], what="topk_merge_packed")
    assert same_bits(res2["val"], res["val"]) and same_bits(res2["idx"], res["idx"])
    assert np.array_equal(res2["status"].cpu().numpy(), status.max(0))
    o2 = ops.topk_merge_packed(torch.stack(packed), return_status=True)
    assert all(same_bits(a, b) for a, b in zip((res2["val"], res2["idx"], res2["status"]), o2))


@covers("gdr_sim_topk")
@pytest.mark.parametrize("d", [64, 128], ids=["gemm", "stream"])
def test_sim_topk_overflow_of_one_query_leaves_the_others_exact(dev, d):
    """A corpus that is degenerate for query 1 only, out of three: column 0 of every document is exactly 1 and query 1 is the unit
    vector e0, so all 60 001 documents tie at score 1 for it and its candidate list overflows; queries 0 and 2 have a zero in
    column 0 and see an ordinary corpus.  With exact_on_overflow=False the status is [0, 1, 0] and queries 0 and 2 equal the
    oracle — an overflowing neighbour must cost them nothing."""
    from conftest import order_insensitive_topk_match
    from oracle import retrieval_ref
    N, k = 60001, 50
    D = synth.make_corpus(N, d, seed=2)
    D[:, 0] = 1.0
    Q, _ = synth.make_queries(D, 3, seed=6)
    Q[:, 0] = 0.0
    Q[1] = 0.0
    Q[1, 0] = 1.0
    assert np.array_equal(Q[1] @ D.T, np.ones(N, np.float32))
    Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
    Qd, qh = guarded_input(Qt, tail=torch.full((128, d), 1e3))
    Dd, dh = guarded_input(Dt, tail=_winning_rows(Q, D, 256))
    need = lib().gdr_sim_topk_workspace_bytes(3, N, d, k, 0)
    keep = torch.tensor([0, 2], device=dev)
    res = run_guarded(dev, {"val": ((3, k), torch.float32), "idx": ((3, k), torch.int32), "status": ((3,), torch.int32)}, need,
                      lambda o, ws, n: lib().gdr_sim_topk(ptr(Qd), 3, ptr(Dd), N, d, k, 0, ptr(o["val"]), ptr(o["idx"]), ptr(o["status"]), 0,
                                                          ptr(ws), n, stream_ptr()), inputs=[qh, dh], what="mixed overflow",
                      project=lambda r: {"val": r["val"][keep], "idx": r["idx"][keep], "status": r["status"]})
    assert res["status"].cpu().tolist() == [0, 1, 0]
    ov, oi, ost = ops.sim_topk(Qt.to(dev), Dt.to(dev), k, return_status=True, exact_on_overflow=False)
    assert ost.cpu().tolist() == [0, 1, 0] and same_bits(ov[keep], res["val"]) and same_bits(oi[keep], res["idx"])
    rv, ri = retrieval_ref.sim_topk(Qt[[0, 2]], Dt, k)
    order_insensitive_topk_match(rv.numpy(), ri.numpy(), res["val"].cpu().numpy(), res["idx"].cpu().numpy().astype(np.int64), TOL)
    # the repaired default: query 1 gets the tie rule's answer (the lowest ids), the others keep their bits
    fv, fi = ops.sim_topk(Qt.to(dev), Dt.to(dev), k)
    assert fi[1].cpu().tolist() == list(range(k)) and same_bits(fv[keep], res["val"]) and same_bits(fi[keep], res["idx"])


# ================================================================================================ rerank and clusters
def _rerank_inputs(bf16):
    """Ragged candidate segments as tests/test_gpu_parity.py::test_rerank_random_ragged_vs_oracle builds them, plus: query 3 has
    fewer than k candidates, query 5 has more than max_cand (the surplus is ignored), and document HOT — in range, never a real
    candidate — would take rank 1 of every list: it fills everything BEHIND the live part of the candidate arrays."""
    rng = np.random.Generator(np.random.PCG64(17))
    B, R, N, d, k, max_cand = 7, 5, 3000, 768, 12, 128
    D = synth.make_corpus(N, d, seed=21)
    Q, _ = synth.make_queries(D, B, seed=22)
    Q *= 0.1                                      # keep tanh / sigmoid away from saturation: ties would hide id errors
    hot = N - 1
    D[hot] = _winning_rows(Q, D, 1, bf16)[0].numpy() * 0.2       # twice the largest real score for every query, not saturated
    if bf16:
        D = torch.from_numpy(D).bfloat16().float().numpy()        # the reference sees the rounded corpus
    s = Q.astype(np.float64) @ D.astype(np.float64).T
    assert (s[:, hot] > 1.5 * np.delete(s, hot, axis=1).max(1)).all() and s[:, hot].max() < 3.0
    segs = []
    for b in range(B):
        row = []
        for j in range(R):
            n = 0 if (b + j) % 4 == 0 else int(rng.integers(1, 26))
            if b == 3:
                n = min(n, 2)
            if b == 5:
                n = 40
            row.append(rng.integers(0, hot, n).astype(np.int32))
        segs.append(row)
    beam = rng.standard_normal((B, R)).astype(np.float32)
    assert sum(len(s) for s in segs[5]) > max_cand and all(sum(len(s) for s in segs[b]) <= max_cand for b in range(B) if b != 5)
    assert 0 < sum(len(s) for s in segs[3]) < k
    return B, R, N, d, k, max_cand, hot, Q, D, segs, beam


@covers("gdr_rerank_topk", "gdr_rerank_topk_bf16", "gdr_rerank_workspace_bytes")
@pytest.mark.parametrize("layout", ["one_csr", "query_blocks"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("func", ["tanh", "sigmoid"])
def test_rerank_topk(dev, layout, bf16, func):
    from oracle import retrieval_ref
    B, R, N, d, k, max_cand, hot, Q, D, segs, beam = _rerank_inputs(bf16)
    alphas = [0, 0.5, 1, 2, 3]
    A = len(alphas)
    pad = 256
    if layout == "one_csr":
        stride = 0
        flat = np.concatenate([s for row in segs for s in row])
        offs = np.concatenate([[0], np.cumsum([len(s) for row in segs for s in row])]).astype(np.int32)
        ids_t, ids_tail = torch.from_numpy(flat), torch.full((pad,), hot, dtype=torch.int32)
        offs_tail = torch.from_numpy(offs[-1] + 7 * np.arange(1, pad + 1, dtype=np.int32))   # as if more beams followed
    else:
        stride = 256                                                                         # >= max_cand, >= the longest list
        offs = np.zeros((B, R + 1), np.int32)
        blocks = np.full((B, stride), hot, np.int32)                                         # HOT behind every query's live part
        for b in range(B):
            row = np.concatenate(segs[b]) if segs[b] else np.zeros(0, np.int32)
            offs[b, 1:] = np.cumsum([len(s) for s in segs[b]])
            blocks[b, :len(row)] = row
        ids_t, ids_tail = torch.from_numpy(blocks), torch.full((stride,), hot, dtype=torch.int32)
        offs_tail = torch.from_numpy(np.tile(np.arange(R + 1, dtype=np.int32) * 40, 8))
    Dt = torch.from_numpy(D)
    d_tail = _winning_rows(Q, D, 64, bf16)
    if bf16:
        Dt, d_tail = Dt.bfloat16(), d_tail.bfloat16()
    Qd, qh = guarded_input(torch.from_numpy(Q), tail=torch.full((64, d), 1e3))
    Dd, dh = guarded_input(Dt, tail=d_tail)
    Od, oh = guarded_input(torch.from_numpy(offs), tail=offs_tail)
    Id, ih = guarded_input(ids_t, tail=ids_tail)
    Bd, bh = guarded_input(torch.from_numpy(beam), tail=torch.full((256,), 1e3))
    Ad, ah = guarded_input(torch.tensor(alphas, dtype=torch.float32), tail=torch.full((256,), 1e3))
    need = lib().gdr_rerank_workspace_bytes(B, max_cand)
    assert need == -(-B * max_cand * 4 // 256) * 256
    fn = lib().gdr_rerank_topk_bf16 if bf16 else lib().gdr_rerank_topk
    fcode = 0 if func == "tanh" else 1
    res = run_guarded(dev, {"val": ((B, A, k), torch.float32), "idx": ((B, A, k), torch.int32)}, need,
                      lambda o, ws, n: fn(ptr(Qd), ptr(Dd), d, ptr(Od), ptr(Id), ptr(Bd), B, R, ptr(Ad), A, k, fcode, ptr(o["val"]),
                                          ptr(o["idx"]), max_cand, stride, 0, N, 0, ptr(ws), n, stream_ptr()),
                      inputs=[qh, dh, oh, ih, bh, ah], what=f"rerank {layout}")
    v, i = res["val"], res["idx"]
    assert not bool((i == hot).any()), "the document behind the live candidates was ranked"
    assert int(i.max()) < N and not bool(torch.isnan(v).any())
    ov, oi = ops.rerank_topk(torch.from_numpy(Q).to(dev), Dt.to(dev), torch.from_numpy(offs).to(dev), ids_t.to(dev),
                             torch.from_numpy(beam).to(dev), alphas, k, func=func, max_cand=max_cand, cand_stride=stride)
    assert same_bits(v, ov) and same_bits(i, oi)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    for b in range(B):
        mem, nums, left = [], [], max_cand                          # candidates past max_cand are ignored (include/gdr_hip.h)
        for s in segs[b]:
            take = s[:left]
            left -= len(take)
            mem += take.tolist()
            nums.append(len(take))
        kk = min(k, len(mem))
        ref = retrieval_ref.rerank(torch.from_numpy(Q[b:b + 1]), torch.from_numpy(D), [mem], [nums], beam[b:b + 1].tolist(), alphas, kk,
                                   func=func)[0]
        for a in range(A):
            rv, ri = ref[a]
            np.testing.assert_allclose(v[b, a, :kk], rv.numpy(), rtol=TOL, atol=TOL)
            same = np.abs(np.diff(rv.numpy())) > 4 * TOL          # ids exact where neighbouring scores are apart
            ok = np.r_[True, same] & np.r_[same, True]
            assert np.array_equal(i[b, a, :kk][ok], ri.numpy()[ok])
            assert (i[b, a, kk:] == -1).all() and np.isneginf(v[b, a, kk:]).all()


@covers("gdr_rerank_wire_pack", "gdr_rerank_wire_unpack", "gdr_rerank_positions_to_ids")
@pytest.mark.parametrize("B,d,R,stride", [(1, 4, 1, 1), (7, 768, 5, 131), (33, 64, 100, 1200)])
def test_rerank_wire_and_positions(dev, B, d, R, stride):
    rng = np.random.default_rng(B + d + R)
    q = rng.standard_normal((B, d)).astype(np.float32)
    beam = rng.standard_normal((B, R)).astype(np.float32)
    offs = np.sort(rng.integers(0, stride + 1, (B, R + 1)).astype(np.int32), axis=1)
    ids = rng.integers(0, 1 << 30, (B, stride)).astype(np.int32)
    tails = lambda dt, n: torch.full((n,), 77, dtype=dt)                                   # noqa: E731
    Qd, qh = guarded_input(torch.from_numpy(q), tail=tails(torch.float32, d * 4))
    Bd, bh = guarded_input(torch.from_numpy(beam), tail=tails(torch.float32, R * 4))
    Od, oh = guarded_input(torch.from_numpy(offs), tail=tails(torch.int32, (R + 1) * 4))
    Id, ih = guarded_input(torch.from_numpy(ids), tail=tails(torch.int32, stride * 4))
    W = d + 2 * R + 1 + stride
    wire = run_guarded(dev, {"wire": ((B, W), torch.int32)}, 0,
                       lambda o, ws, n: lib().gdr_rerank_wire_pack(ptr(Qd), ptr(Bd), ptr(Od), ptr(Id), B, d, R, stride, ptr(o["wire"]),
                                                                   stream_ptr()), inputs=[qh, bh, oh, ih], what="wire_pack")["wire"]
    want = np.concatenate([q.view(np.int32), beam.view(np.int32), offs, ids], axis=1)
    assert np.array_equal(wire.cpu().numpy(), want)
    assert same_bits(wire, ops.rerank_wire_pack(*[torch.from_numpy(x).to(dev) for x in (q, beam, offs, ids)]))
    Wd, wh = guarded_input(torch.from_numpy(want), tail=tails(torch.int32, W * 4))
    un = run_guarded(dev, {"q": ((B, d), torch.float32), "beam": ((B, R), torch.float32), "offs": ((B, R + 1), torch.int32),
                           "ids": ((B, stride), torch.int32)}, 0,
                     lambda o, ws, n: lib().gdr_rerank_wire_unpack(ptr(Wd), B, d, R, stride, ptr(o["q"]), ptr(o["beam"]), ptr(o["offs"]),
                                                                   ptr(o["ids"]), stream_ptr()), inputs=[wh], what="wire_unpack")
    for got, src in zip((un["q"], un["beam"], un["offs"], un["ids"]), (q, beam, offs, ids)):
        assert same_bits(got, torch.from_numpy(src).to(dev))
    # merged candidate positions -> doc ids through the query's own block; negative positions stay -1
    per_query = 3 * 25
    pos = rng.integers(-1, stride, (B, per_query)).astype(np.int32)
    Pd, ph = guarded_input(torch.from_numpy(pos), tail=torch.zeros(1024, dtype=torch.int32))
    out = run_guarded(dev, {"ids": ((B, per_query), torch.int32)}, 0,
                      lambda o, ws, n: lib().gdr_rerank_positions_to_ids(ptr(Pd), ptr(Id), B, per_query, stride, ptr(o["ids"]), stream_ptr()),
                      inputs=[ph, ih], what="positions_to_ids")["ids"]
    want_ids = np.where(pos >= 0, np.take_along_axis(ids, np.maximum(pos, 0), axis=1), -1)
    assert np.array_equal(out.cpu().numpy(), want_ids)
    assert same_bits(out, ops.rerank_positions_to_ids(torch.from_numpy(pos).to(dev), torch.from_numpy(ids).to(dev)))


@covers("gdr_cluster_candidates")
def test_cluster_candidates(dev):
    """The device lookup of tests/test_gpu_rerank.py::test_cluster_candidates_device_equals_host_lookup with guarded outputs; the
    rows behind out_ids name a real cluster (valid tokens), the entries of a candidate block behind its live part are not part
    of the contract and are left out of the comparison."""
    from gdr_amd import codec
    from test_gpu_rerank import _index, _rows_for
    V, ml, B, R = 30, 10, 9, 6
    index, names, depth = _index(7003, 12, V)
    rng = np.random.Generator(np.random.PCG64(1))
    picks = [int(rng.integers(0, len(names))) for _ in range(B * R)]
    picks[3] = picks[2]
    picks[7], picks[13], picks[20] = "unknown", "noeos", "empty"
    picks[R * 4:R * 5] = ["unknown"] * R
    rows = _rows_for(names, picks, V, ml, rng)
    tail_rows = _rows_for(names, [0] * 64, V, ml, rng)
    dec = codec.dec_2d(codec.decode_token(rows, kary=V, output_vocab_size=V), R)
    offs_h, ids_h, max_h = index.candidates(dec)
    offs_h, ids_h = offs_h.numpy(), ids_h.numpy()
    dci = ops.DeviceClusterIndex(index, dev, V)
    stride = R * dci.max_cluster
    Rd, rh = guarded_input(torch.from_numpy(rows), tail=torch.from_numpy(tail_rows))

    def live(r):
        n = r["offs"][:, R:R + 1].long()
        cols = torch.arange(stride, device=dev)[None, :]
        return {"cl": r["cl"], "offs": r["offs"], "ids": torch.where(cols < n, r["ids"], torch.zeros_like(r["ids"]))}

    res = run_guarded(dev, {"cl": ((B * R,), torch.int32), "offs": ((B, R + 1), torch.int32), "ids": ((B, stride), torch.int32)}, 0,
                      lambda o, ws, n: lib().gdr_cluster_candidates(C.byref(dci.struct), ptr(Rd), B, R, ml, ptr(o["cl"]), ptr(o["offs"]),
                                                                    ptr(o["ids"]), stride, stream_ptr()), inputs=[rh], what="cluster_candidates",
                      project=live)
    cl, offs, ids = (res[n].cpu().numpy() for n in ("cl", "offs", "ids"))
    for b in range(B):
        base = offs_h[b * R]
        assert np.array_equal(offs[b], offs_h[b * R:(b + 1) * R + 1] - base), b
        n = offs[b, R]
        assert np.array_equal(ids[b, :n], ids_h[base:base + n]), b
    assert cl.tolist() == [index.lookup.get(s, -1) for row in dec for s in row]
    o_cl, o_offs, o_ids, o_stride = dci.candidates(torch.from_numpy(rows).to(dev), B, R)
    got = live({"cl": o_cl, "offs": o_offs, "ids": o_ids})
    assert o_stride == stride and all(same_bits(res[n], got[n]) for n in res)


def _csr(rng, sizes, N):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mem = np.concatenate([np.sort(rng.choice(N, s, replace=False)) for s in sizes] + [np.zeros(0, np.int64)]).astype(np.int32)
    return off, mem


@covers("gdr_cluster_centroids")
@pytest.mark.parametrize("d", [4, 96, 768])
def test_cluster_centroids(dev, d):
    import expand_ref
    rng = np.random.default_rng(d)
    N = 3001
    X = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float32)
    sizes = [12, 0, 1, 300, 7, 0, 65, 64]
    off, mem = _csr(rng, sizes, N)
    Dd, dh = guarded_input(torch.from_numpy(X), tail=torch.full((64, d), 1e6))
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.from_numpy(off[-1] + 5 * np.arange(1, 257, dtype=np.int32)))
    Md, mh = guarded_input(torch.from_numpy(mem), tail=torch.full((1024,), N - 1, dtype=torch.int32))     # in-range ids behind the members
    Cn = len(sizes)
    res = run_guarded(dev, {"cent": ((Cn, d), torch.float32), "counts": ((Cn,), torch.int32)}, 0,
                      lambda o, ws, n: lib().gdr_cluster_centroids(ptr(Dd), N, d, ptr(Od), ptr(Md), len(mem), Cn, ptr(o["cent"]),
                                                                   ptr(o["counts"]), stream_ptr()), inputs=[dh, oh, mh], what="cluster_centroids")
    want, counts = expand_ref.centroids(X, off, mem)
    assert np.array_equal(res["cent"].cpu().numpy().view(np.uint32), want.view(np.uint32)), "not the reference's sequential fp32 mean"
    assert res["counts"].cpu().tolist() == sizes == counts.tolist()
    oc, on = ops.cluster_centroids_csr(torch.from_numpy(X).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(mem).to(dev))
    assert same_bits(res["cent"], oc) and same_bits(res["counts"], on)


@covers("gdr_cluster_insert", "gdr_cluster_insert_workspace_bytes")
@pytest.mark.parametrize("with_map", [False, True], ids=["direct", "target_map"])
def test_cluster_insert(dev, with_map):
    import expand_ref
    rng = np.random.default_rng(5)
    Cn, N0, n_new = 301, 5000, 9000                          # cluster 7 receives more than 4 096 documents: the ordered pass
    sizes = rng.multinomial(N0, np.ones(Cn) / Cn)
    sizes[3] = 0
    sizes[-1] += N0 - sizes.sum()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mem = rng.permutation(N0).astype(np.int32)
    new_ids = np.arange(N0, N0 + n_new, dtype=np.int32)
    cluster = rng.integers(0, Cn, n_new).astype(np.int32)
    cluster[:5000] = 7
    if with_map:
        cmap = np.array([c for c in range(Cn) if c != 3], np.int32)     # compact index -> cluster (the empty one has no centroid)
        cluster = np.where(cluster == 3, 4, cluster)
        target = np.searchsorted(cmap, cluster).astype(np.int32)
    else:
        cmap, target = None, cluster
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.full((256,), N0, dtype=torch.int32))
    Md, mh = guarded_input(torch.from_numpy(mem), tail=torch.arange(1024, dtype=torch.int32))
    Nd, nh = guarded_input(torch.from_numpy(new_ids), tail=torch.arange(N0 + n_new, N0 + n_new + 1024, dtype=torch.int32))
    Td, th = guarded_input(torch.from_numpy(target), tail=torch.full((1024,), 7, dtype=torch.int32))      # valid targets behind the last one
    handles = [oh, mh, nh, th]
    Pd = None
    if with_map:
        Pd, ph = guarded_input(torch.from_numpy(cmap), tail=torch.full((256,), 7, dtype=torch.int32))
        handles.append(ph)
    need = lib().gdr_cluster_insert_workspace_bytes(Cn)
    res = run_guarded(dev, {"off": ((Cn + 1,), torch.int32), "mem": ((N0 + n_new,), torch.int32), "max": ((1,), torch.int32)}, need,
                      lambda o, ws, n: lib().gdr_cluster_insert(ptr(Od), ptr(Md), Cn, N0, ptr(Nd), ptr(Td), n_new, ptr(Pd),
                                                                len(cmap) if with_map else 0, ptr(o["off"]), ptr(o["mem"]), ptr(o["max"]),
                                                                ptr(ws), n, stream_ptr()), inputs=handles, what="cluster_insert")
    want_off, want_mem = expand_ref.merge(off, mem, new_ids, cluster)
    assert np.array_equal(res["off"].cpu().numpy(), want_off) and np.array_equal(res["mem"].cpu().numpy(), want_mem)
    assert int(res["max"][0]) == int(np.diff(want_off).max())
    o_off, o_mem, o_max = ops.cluster_insert(*[torch.from_numpy(x).to(dev) for x in (off, mem, new_ids, target)],
                                             target_map=torch.from_numpy(cmap).to(dev) if with_map else None)
    assert same_bits(res["off"], o_off) and same_bits(res["mem"], o_mem) and o_max == int(res["max"][0])


# ================================================================================================ k-means level kernels
def _kmeans_level(rng, N, sizes):
    perm = rng.permutation(N)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(perm[off[i]:off[i + 1]]) for i in range(len(sizes))]).astype(np.int32)
    return off, rows


@covers("gdr_kmeans_assign", "gdr_kmeans_assign_workspace_bytes", "gdr_kmeans_assign_tile")
@pytest.mark.parametrize("d,k", [(768, 30), (64, 2), (100, 64)])
def test_kmeans_assign(dev, d, k):
    rng = np.random.default_rng(9 + d)
    N = 9000
    X = synth.make_corpus(N, d, seed=6)
    sizes = [2500, 31, 900, 129, 3000, 64, 1]
    S, n = len(sizes), sum(sizes)
    off, rows = _kmeans_level(rng, N, sizes)
    cent = np.concatenate([X[rng.choice(rows[off[i]:off[i + 1]], k, replace=len(rows[off[i]:off[i + 1]]) < k)] for i in range(S)])
    work = ops.kmeans_worklist(torch.from_numpy(off).to(dev), lib().gdr_kmeans_assign_tile()).cpu()
    prev = rng.integers(0, k, n).astype(np.int32)
    Dd, dh = guarded_input(torch.from_numpy(X), tail=torch.full((64, d), 1e3))                 # a row id >= N reads as a ZERO row, not these
    Rd, rh = guarded_input(torch.from_numpy(rows), tail=torch.full((1024,), N - 1, dtype=torch.int32))
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.full((256,), n, dtype=torch.int32))
    Cd, ch = guarded_input(torch.from_numpy(cent), tail=torch.full((64, d), 1e3))             # centroids behind the last node's
    Wd, wh = guarded_input(work, tail=torch.tensor([[S - 1, int(off[-2])]] * 256, dtype=torch.int32))   # well-formed items behind the list
    Pd, ph = guarded_input(torch.from_numpy(prev), tail=torch.zeros(1024, dtype=torch.int32))
    need = lib().gdr_kmeans_assign_workspace_bytes(S, k)
    res = run_guarded(dev, {"lab": ((n,), torch.int32), "score": ((n,), torch.float32), "changed": ((S,), torch.int32),
                            "status": ((1,), torch.int32)}, need,
                      lambda o, ws, nb: lib().gdr_kmeans_assign(ptr(Dd), N, d, ptr(Rd), n, ptr(Od), S, ptr(Cd), k, ptr(Wd), work.shape[0], ptr(Pd),
                                                                ptr(o["lab"]), ptr(o["score"]), ptr(o["changed"]), ptr(o["status"]), ptr(ws), nb,
                                                                stream_ptr()), inputs=[dh, rh, oh, ch, wh, ph], what="kmeans_assign")
    lab, sc = res["lab"].cpu().numpy(), res["score"].cpu().numpy()
    assert int(res["status"][0]) == 0 and lab.min() >= 0 and lab.max() < k and not np.isnan(sc).any()
    # tests/test_gpu_kmeans.py: every row's chosen score within the fp32 band of the float64 maximum
    X64 = X.astype(np.float64)
    for i in range(S):
        C64 = cent[i * k:(i + 1) * k].astype(np.float64)
        r = rows[off[i]:off[i + 1]]
        s = X64[r] @ C64.T - 0.5 * (C64 * C64).sum(1)[None, :]
        band = (2 * d + 8) * 2.0 ** -24 * np.linalg.norm(X64[r], axis=1) * np.linalg.norm(C64, axis=1).max()
        chosen = s[np.arange(len(r)), lab[off[i]:off[i + 1]]]
        assert (s.max(1) - chosen <= band).all() and (np.abs(sc[off[i]:off[i + 1]] - chosen) <= band).all(), f"node {i}"
        assert int(res["changed"][i]) == int((lab[off[i]:off[i + 1]] != prev[off[i]:off[i + 1]]).sum())
    o = ops.kmeans_assign(torch.from_numpy(X).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev),
                          torch.from_numpy(cent).to(dev), k, prev_labels=torch.from_numpy(prev).to(dev))
    assert all(same_bits(res[nm], t) for nm, t in zip(("lab", "score", "changed", "status"), o))


@covers("gdr_kmeans_partition", "gdr_kmeans_partition_workspace_bytes", "gdr_kmeans_partition_tile")
@pytest.mark.parametrize("k,sizes", [(30, [70000, 1, 255, 256, 257, 31, 5000]), (64, [3, 1000]), (2, [513])])
def test_kmeans_partition(dev, k, sizes):
    rng = np.random.default_rng(2)
    n, S = sum(sizes), len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(rng.choice(10 ** 6, s, replace=False)) for s in sizes]).astype(np.int32)
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[off[-2]:off[-1]][::2] = k - 1
    work = ops.kmeans_worklist(torch.from_numpy(off).to(dev), lib().gdr_kmeans_partition_tile()).cpu()
    Rd, rh = guarded_input(torch.from_numpy(rows), tail=torch.arange(1024, dtype=torch.int32))
    Ld, lh = guarded_input(torch.from_numpy(lab), tail=torch.zeros(1024, dtype=torch.int32))           # valid labels behind the last row
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.full((256,), n, dtype=torch.int32))
    Wd, wh = guarded_input(work, tail=torch.tensor([[S - 1, int(off[-2])]] * 256, dtype=torch.int32))
    need = lib().gdr_kmeans_partition_workspace_bytes(work.shape[0], k)
    res = run_guarded(dev, {"rows": ((n,), torch.int32), "child": ((S * k + 1,), torch.int32), "status": ((1,), torch.int32)}, need,
                      lambda o, ws, nb: lib().gdr_kmeans_partition(ptr(Rd), ptr(Ld), n, ptr(Od), S, k, ptr(Wd), work.shape[0], ptr(o["rows"]),
                                                                   ptr(o["child"]), ptr(o["status"]), ptr(ws), nb, stream_ptr()),
                      inputs=[rh, lh, oh, wh], what="kmeans_partition")
    er, eo = [], [0]
    for i in range(S):
        r, l = rows[off[i]:off[i + 1]], lab[off[i]:off[i + 1]]
        for j in range(k):
            er.append(r[l == j])
            eo.append(eo[-1] + len(er[-1]))
    assert int(res["status"][0]) == 0
    assert np.array_equal(res["child"].cpu().numpy(), np.array(eo, np.int32)) and np.array_equal(res["rows"].cpu().numpy(), np.concatenate(er))
    o = ops.kmeans_partition(torch.from_numpy(rows).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(off).to(dev), k)
    assert all(same_bits(res[nm], t) for nm, t in zip(("rows", "child", "status"), o))


@covers("gdr_kmeans_centroids", "gdr_kmeans_centroids_workspace_bytes")
@pytest.mark.parametrize("d", [96, 768])
def test_kmeans_centroids(dev, d):
    import kmeans_ref as kr
    rng = np.random.default_rng(8)
    N = 6000
    X = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float32)
    sizes = [1000, 0, 3, 256, 257, 600, 1, 0, 513, 255, 2048, 0]
    off, rows = _csr(rng, sizes, N)
    n, Cn = len(rows), len(sizes)
    Dd, dh = guarded_input(torch.from_numpy(X), tail=torch.full((64, d), 1e6))
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.from_numpy(off[-1] + 300 * np.arange(1, 257, dtype=np.int32)))
    Rd, rh = guarded_input(torch.from_numpy(rows), tail=torch.full((4096,), N - 1, dtype=torch.int32))
    need = lib().gdr_kmeans_centroids_workspace_bytes(n, d)
    res = run_guarded(dev, {"cent": ((Cn, d), torch.float32), "counts": ((Cn,), torch.int32)}, need,
                      lambda o, ws, nb: lib().gdr_kmeans_centroids(ptr(Dd), N, d, ptr(Od), ptr(Rd), n, Cn, ptr(o["cent"]), ptr(o["counts"]),
                                                                   ptr(ws), nb, stream_ptr()), inputs=[dh, oh, rh], what="kmeans_centroids")
    cent = res["cent"].cpu().numpy()
    assert res["counts"].cpu().tolist() == sizes
    for c, sz in enumerate(sizes):
        if sz == 0:
            assert not cent[c].any()
        else:
            want = kr.two_stage_mean(X, rows[off[c]:off[c + 1]])
            assert np.array_equal(cent[c].view(np.uint32), want.view(np.uint32)), f"child {c} ({sz} members)"
    oc, on = ops.kmeans_centroids(torch.from_numpy(X).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(rows).to(dev))
    assert same_bits(res["cent"], oc) and same_bits(res["counts"], on)


# ================================================================================================ models
from gdr_amd.config import GDRConfig   # noqa: E402


@functools.lru_cache(maxsize=2)
def _t5_setup(kind):
    cfg = GDRConfig.tiny() if kind == "tiny" else GDRConfig.base(num_layers=2)      # base widths, two blocks: every linear shape
    sd = synth.make_state_dict(cfg, seed=77, with_decoder=False)
    return cfg, sd


@functools.lru_cache(maxsize=2)
def _t5_oracle(kind, B, L, bf16):
    from oracle import t5_ref
    cfg, sd = _t5_setup(kind)
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=5 + B, min_len=max(1, L // 5))
    if bf16:
        with t5_ref.bf16_linears():
            return t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))
    return t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))


# form -> (handle kwargs, workspace-size function, entry point, ragged, extra trailing ints before the workspace)
T5_FORMS = {
    "padded": ({}, "gdr_t5_encoder_workspace_bytes", "gdr_t5_encoder_forward", False),
    "ragged": ({}, "gdr_t5_encoder_ragged_workspace_bytes", "gdr_t5_encoder_forward_ragged", True),
    "padded_bf16": (dict(dtype=torch.bfloat16), "gdr_t5_encoder_bf16_workspace_bytes", "gdr_t5_encoder_forward_bf16", False),
    "ragged_bf16": (dict(dtype=torch.bfloat16), "gdr_t5_encoder_ragged_workspace_bytes", "gdr_t5_encoder_forward_ragged_bf16", True),
    "ragged_split6": (dict(split=6), "gdr_t5_encoder_split_workspace_bytes", "gdr_t5_encoder_forward_ragged_split", True),
    "ragged_split2": (dict(split=2), "gdr_t5_encoder_split_workspace_bytes", "gdr_t5_encoder_forward_ragged_split", True),
}


@covers("gdr_t5_encoder_forward", "gdr_t5_encoder_forward_ragged", "gdr_t5_encoder_forward_bf16", "gdr_t5_encoder_forward_ragged_bf16",
        "gdr_t5_encoder_forward_ragged_split", "gdr_t5_encoder_workspace_bytes", "gdr_t5_encoder_ragged_workspace_bytes",
        "gdr_t5_encoder_bf16_workspace_bytes", "gdr_t5_encoder_split_workspace_bytes")
@pytest.mark.parametrize("form,kind,B,L", [
    (f, kind, B, L) for kind, B, L in [("tiny", 3, 5), ("tiny", 7, 40), ("base2", 4, 40), ("base2", 48, 40), ("base2", 120, 40)]
    for f in T5_FORMS if not ("split" in f and kind == "tiny")],     # the split form needs d_kv = 64 and widths % 64 == 0: base only
    ids=lambda v: str(v))
def test_t5_encoder_forms(dev, form, kind, B, L):
    """The five encoder entry points at B*L below 256 (the ragged entries run the padded form), below 4 096 (packed rows on the
    split-K / stream-K linears) and above (packed rows, whole tiles).  Valid token ids and ones follow ids / mask."""
    hkw, ws_fn, entry, ragged = T5_FORMS[form]
    cfg, sd = _t5_setup(kind)
    enc = ops.T5EncoderHandle(cfg, sd, dev, **hkw)
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=5 + B, min_len=max(1, L // 5))
    Id, ih = guarded_input(torch.from_numpy(ids), tail=torch.full((8 * L,), 7, dtype=torch.int64))
    Md, mh = guarded_input(torch.from_numpy(mask), tail=torch.ones(8 * L, dtype=torch.int64))
    need = getattr(lib(), ws_fn)(C.byref(enc.dims), B, L)
    fn = getattr(lib(), entry)
    d = cfg.d_model
    live = int(mask.sum())

    def call(o, ws, n, hint=-1, hidden=True):
        hp = ptr(o["hidden"]) if hidden else None
        if not ragged:
            return fn(C.byref(enc.struct), ptr(Id), ptr(Md), B, L, hp, ptr(o["pooled"]), ptr(ws), n, stream_ptr())
        if "split" in form:
            return fn(C.byref(enc.struct), ptr(Id), ptr(Md), B, L, hp, ptr(o["pooled"]), hint, enc.split, ptr(ws), n, stream_ptr())
        return fn(C.byref(enc.struct), ptr(Id), ptr(Md), B, L, hp, ptr(o["pooled"]), hint, ptr(ws), n, stream_ptr())

    specs = {"hidden": ((B, L, d), torch.float32), "pooled": ((B, d), torch.float32)}
    res = run_guarded(dev, specs, need, call, inputs=[ih, mh], what=f"{entry} {kind} {B}x{L}")
    h, p = res["hidden"], res["pooled"]
    oh_, op_ = enc.forward(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), ragged=ragged)
    assert same_bits(h, oh_) and same_bits(p, op_), "differs from the ops path"
    assert same_bits(p, h[:, 0].contiguous())
    keep = torch.from_numpy(mask != 0)
    if ragged:
        assert int((h.cpu()[~keep] != 0).sum()) == 0, "dropped rows of the ragged form must be zero"
        # the row hint is a tuning input; a pooled-only call carries the CLS rows alone through the last block
        hinted = run_guarded(dev, specs, need, lambda o, ws, n: call(o, ws, n, hint=live), inputs=[ih, mh], fills=(0x5A,), what="row hint")
        assert same_bits(hinted["hidden"], h) and same_bits(hinted["pooled"], p)
        pooled_only = run_guarded(dev, {"pooled": ((B, d), torch.float32)}, need, lambda o, ws, n: call(o, ws, n, hidden=False),
                                  inputs=[ih, mh], fills=(0xFF, 0x5A), what="pooled only")["pooled"]
        if form == "ragged":
            assert same_bits(pooled_only, p)
        else:                                                        # bf16 / split: the bound of the doc tower's sibling tests
            assert float((pooled_only - p).abs().max()) <= 1e-5
    hc = h.cpu()
    if "bf16" in form:
        ref16 = _t5_oracle(kind, B, L, True)
        if kind == "tiny":
            torch.testing.assert_close(hc[keep], ref16[keep], rtol=5e-3, atol=5e-3)
        else:
            assert float((hc[keep] - ref16[keep]).norm() / ref16[keep].norm()) < 8e-3 and float((hc[keep] - ref16[keep]).abs().max()) < 6e-2
        torch.testing.assert_close(hc[keep], _t5_oracle(kind, B, L, False)[keep], rtol=1e-1, atol=1e-1)
    else:
        tol = TOL if kind == "tiny" else 2e-4
        torch.testing.assert_close(hc[keep], _t5_oracle(kind, B, L, False)[keep], rtol=tol, atol=tol)


def _bert_tokens(lens, L, vocab, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens)
    ids = g.integers(2, vocab, size=(len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids[np.arange(len(lens)), lens - 1] = 1
    return ids * mask, mask


BERT_FORMS = {
    "padded": ({}, "gdr_bert_encoder_workspace_bytes", "gdr_bert_encoder_forward", False),
    "ragged": ({}, "gdr_bert_encoder_ragged_workspace_bytes", "gdr_bert_encoder_forward_ragged", True),
    "ragged_bf16": (dict(dtype=torch.bfloat16), "gdr_bert_encoder_ragged_workspace_bytes", "gdr_bert_encoder_forward_ragged_bf16", True),
    "ragged_split": (dict(split=True), "gdr_bert_encoder_ragged_workspace_bytes", "gdr_bert_encoder_forward_ragged_split", True),
}


@covers("gdr_bert_encoder_forward", "gdr_bert_encoder_forward_ragged", "gdr_bert_encoder_forward_ragged_bf16",
        "gdr_bert_encoder_forward_ragged_split", "gdr_bert_encoder_workspace_bytes", "gdr_bert_encoder_ragged_workspace_bytes")
@pytest.mark.parametrize("form", list(BERT_FORMS))
@pytest.mark.parametrize("L", [40, 128, 200])
@pytest.mark.parametrize("size", ["few_rows", "packed"])
def test_bert_encoder_forms(dev, form, L, size):
    """The four doc-tower entry points at L = 40, 128 and 200 (above 128 tokens: the key-block attention), with a handful of
    passages (the ragged entries run the padded form) and with enough rows for the packed kernels (192 GEMM tiles, bert.hip)."""
    from oracle import bert_ref
    hkw, ws_fn, entry, ragged = BERT_FORMS[form]
    bc = dict(synth.bert_config(True), max_pos=512)
    sd = synth.make_bert_state_dict(bc, seed=77)
    bert = ops.BertEncoderHandle(bc, sd, dev, **hkw)
    B = 5 if size == "few_rows" else -(-(192 * 128 + 128) // L)
    rng = np.random.default_rng(L + B)
    lens = rng.integers(1, L + 1, B)
    lens[:3] = [L, 1, max(1, L - 1)]
    ids, mask = _bert_tokens(lens, L, bc["vocab_size"], seed=1000 + L)
    tt = (np.arange(L)[None, :] >= (lens[:, None] // 2)).astype(np.int64) * mask
    Id, ih = guarded_input(torch.from_numpy(ids), tail=torch.full((8 * L,), 7, dtype=torch.int64))
    Md, mh = guarded_input(torch.from_numpy(mask), tail=torch.ones(8 * L, dtype=torch.int64))
    Td, th = guarded_input(torch.from_numpy(tt), tail=torch.ones(8 * L, dtype=torch.int64))
    need = getattr(lib(), ws_fn)(C.byref(bert.struct), B, L)
    fn = getattr(lib(), entry)
    d = bc["hidden_size"]

    def call(o, ws, n, hidden=True):
        hp = ptr(o["hidden"]) if hidden else None
        if ragged:
            return fn(C.byref(bert.struct), ptr(Id), ptr(Md), ptr(Td), B, L, hp, ptr(o["pooled"]), -1, ptr(ws), n, stream_ptr())
        return fn(C.byref(bert.struct), ptr(Id), ptr(Md), ptr(Td), B, L, hp, ptr(o["pooled"]), ptr(ws), n, stream_ptr())

    specs = {"hidden": ((B, L, d), torch.float32), "pooled": ((B, d), torch.float32)}
    res = run_guarded(dev, specs, need, call, inputs=[ih, mh, th], what=f"{entry} {B}x{L}")
    h, p = res["hidden"], res["pooled"]
    dv = lambda a: torch.from_numpy(a).to(dev)                                               # noqa: E731
    oh_, op_ = bert.forward(dv(ids), dv(mask), dv(tt), ragged=ragged)
    assert same_bits(h, oh_) and same_bits(p, op_), "differs from the ops path"
    pooled_only = run_guarded(dev, {"pooled": ((B, d), torch.float32)}, need, lambda o, ws, n: call(o, ws, n, hidden=False),
                              inputs=[ih, mh, th], fills=(0xFF, 0x5A), what="pooled only")["pooled"]
    keep = mask != 0
    hc, pc = h.cpu().numpy(), p.cpu().numpy()
    if ragged:
        assert not hc[~keep].any(), "PAD rows of the ragged form must be zero"
    sub = np.r_[0:min(B, 40), max(B - 24, 0):B]                                              # the oracle on a subset of the passages
    sub = np.unique(sub)
    kw = dict(bf16=True) if "bf16" in form else {}
    rh, rp = bert_ref.bert_forward(sd, bc, torch.from_numpy(ids[sub]), torch.from_numpy(mask[sub]), token_type_ids=torch.from_numpy(tt[sub]), **kw)
    rh, rp = rh.numpy(), rp.numpy()
    if "bf16" in form:
        dd = np.abs(hc[sub] - rh)[keep[sub]]
        assert dd.max() <= 3e-2 and dd.mean() <= 4e-3 and np.abs(pc[sub] - rp).max() <= 3e-2
        assert float((pooled_only - p).abs().max()) < 1e-5
    else:
        tol = 2e-4 if "split" in form else TOL
        np.testing.assert_allclose(pc[sub], rp, rtol=tol, atol=tol)
        np.testing.assert_allclose(hc[sub][keep[sub]], rh[keep[sub]], rtol=tol, atol=tol)
        if "split" not in form:
            assert same_bits(pooled_only, p)
        else:
            assert float((pooled_only - p).abs().max()) <= 1e-5


def _docids(V, depth, keep_every):
    return ["-".join(str(x) for x in synth.cluster_digits(c, depth, V)) for c in range(V ** depth) if c % keep_every == 0]


class _ExactWorkspace:
    """ops.Workspace look-alike that hands out one guarded buffer and insists on the size it was made for."""

    def __init__(self, view):
        self.view = view

    def get(self, nbytes):
        assert nbytes == self.view.numel(), (nbytes, self.view.numel())
        return self.view


def _prefix_table_dims(dec, trie):
    cfg = dec.cfg
    bfs, level_off, parent, tok = trie.breadth_first()
    n_levels = min(len(level_off) - 1, cfg.max_output_length - 1)
    n_table = int(level_off[n_levels])
    max_n = int(max(level_off[s + 1] - level_off[s] for s in range(n_levels)))
    need = lib().gdr_t5_prefix_table_workspace_bytes(C.byref(dec.struct), max_n)
    return n_table, need


@covers("gdr_t5_prefix_table_build", "gdr_t5_prefix_table_build_bf16", "gdr_t5_prefix_table_workspace_bytes")
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_prefix_table_build(dev, bf16):
    from gdr_amd import codec
    from oracle import t5_ref
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=21)
    V, d, Vd, na = cfg.output_vocab_size, cfg.d_model, cfg.decode_vocab_size, cfg.adaptor_layer_num
    trie = codec.Trie.from_docids(_docids(V, 3, 5), V)
    dec = ops.T5DecoderHandle(cfg, sd, dev, dtype=torch.bfloat16 if bf16 else torch.float32)
    n_table, need = _prefix_table_dims(dec, trie)
    tabs = []

    def call(o, ws, n):
        tabs.append(ops.PrefixTable(dec, trie, dev, kv=o["kv"], W=o["W"], workspace=_ExactWorkspace(ws)))
        return 0

    res = run_guarded(dev, {"kv": ((na, n_table, 3 * d), torch.float32), "W": ((n_table, V + 1, d), torch.float32)}, need, call,
                      what="prefix_table_build")
    plain = ops.PrefixTable(dec, trie, dev)
    assert plain.n_table == n_table and same_bits(res["kv"], plain.kv) and same_bits(res["W"], plain.W)
    # tests/test_gpu_prefix.py: every stored head matrix against the oracle's adaptor + head
    bfs, level_off, parent, tok = trie.breadth_first()
    Wg = res["W"].cpu()
    for s in range(plain.n_levels):
        nodes = list(range(int(level_off[s]), int(level_off[s + 1])))[:7]
        prefixes = []
        for nd in nodes:
            seq, x = [], nd
            while x >= 0:
                seq.append(int(tok[x]))
                x = int(parent[x])
            prefixes.append(seq[::-1])
        ids = torch.tensor(prefixes, dtype=torch.long)
        a = t5_ref.adaptor_forward(sd, cfg, ids)[:, -1]
        cols = t5_ref.valid_columns(s, V)
        Wl = sd["adaptor_linear.weight"].view(d, Vd, d)[:, cols, :]
        ref = torch.einsum("rk,ick->rci", a, Wl) + sd["lm_head.weight"][cols].unsqueeze(0)
        tol = 3e-2 if bf16 else TOL                                  # bf16 mode: SURVEY §8d's 3e-2 (tests/test_gpu_decode.py)
        torch.testing.assert_close(Wg[nodes], ref, rtol=tol, atol=tol)


@covers("gdr_t5_generate", "gdr_t5_generate_bf16", "gdr_t5_generate_workspace_bytes")
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_trie,use_table", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "trie", "table", "trie_table"])
def test_generate(dev, bf16, use_trie, use_table):
    from gdr_amd import codec
    from oracle import beam_ref, codec_ref
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    V, ml = cfg.output_vocab_size, cfg.max_output_length
    docids = _docids(V, 2, 3)
    trie = codec.Trie.from_docids(docids, V)
    B, R, L = 5, 6, 9
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=4, min_len=2)
    dt = torch.bfloat16 if bf16 else torch.float32
    enc, dec = ops.T5EncoderHandle(cfg, sd, dev, dtype=dt), ops.T5DecoderHandle(cfg, sd, dev, dtype=dt)
    tab = ops.PrefixTable(dec, trie, dev) if use_table else None
    dtrie = (tab.device_trie if tab is not None else ops.DeviceTrie(trie, dev)) if use_trie else None
    enc_h, _ = enc.forward(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), want_pooled=False)
    d = cfg.d_model
    Ed, eh = guarded_input(enc_h.cpu(), tail=torch.full((8 * L, d), NAN))                     # NaN states behind the last query's
    Md, mh = guarded_input(torch.from_numpy(mask), tail=torch.ones(8 * L, dtype=torch.int64))
    need = lib().gdr_t5_generate_workspace_bytes(C.byref(dec.struct), B, L, R, ml)
    fn = lib().gdr_t5_generate_bf16 if bf16 else lib().gdr_t5_generate
    specs = {"ids": ((B * R, ml), torch.int64), "len": ((B * R,), torch.int32), "score": ((B * R,), torch.float64)}

    def call(o, ws, n, trace=False):
        return fn(C.byref(dec.struct), ptr(Ed), ptr(Md), B, L, R, ml, 0.8, R, dtrie.struct_ref() if dtrie is not None else None,
                  tab.struct_ref() if tab is not None else None, ptr(o["ids"]), ptr(o["len"]), ptr(o["score"]),
                  ptr(o["ts"]) if trace else None, ptr(o["tt"]) if trace else None, ptr(ws), n, stream_ptr())

    res = run_guarded(dev, specs, need, call, inputs=[eh, mh], what="generate")
    oi, ol, osc = dec.generate(enc_h, torch.from_numpy(mask).to(dev), R, ml, 0.8, R, trie=dtrie, prefix_table=tab)
    assert same_bits(res["ids"], oi) and same_bits(res["len"], ol) and same_bits(res["score"], osc), "differs from the ops path"
    assert not bool(torch.isnan(res["score"]).any())
    # with the per-step trace (no early exit): the same hypotheses
    tspecs = dict(specs, ts=((ml - 1, B, 2 * R), torch.float32), tt=((ml - 1, B, 2 * R), torch.int32))
    tr = run_guarded(dev, tspecs, need, lambda o, ws, n: call(o, ws, n, trace=True), inputs=[eh, mh], fills=(0xFF, 0x5A), what="generate + trace")
    assert all(same_bits(tr[k_], res[k_]) for k_ in specs)
    dec_ids, sc = ops.finish_generate_output(res["ids"], res["len"], res["score"], ml)
    tree = beam_ref.build_trie([codec_ref.encode_single_newid(s, kary=V) for s in docids]) if use_trie else None
    (rd, rs), _ = beam_ref.generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), R, restricted_head=True, decode_tree=tree)
    fin = np.isfinite(np.array(rs))
    if bf16:
        np.testing.assert_allclose(np.array(sc)[fin], np.array(rs)[fin], rtol=3e-2, atol=3e-2)   # bf16 hypothesis scores
    else:
        np.testing.assert_allclose(np.array(sc)[fin], np.array(rs)[fin], rtol=TOL, atol=TOL)
        assert np.array_equal(dec_ids.cpu().numpy()[fin], rd.numpy()[fin])


@covers("gdr_beam_search_table", "gdr_beam_search_table_workspace_bytes")
@pytest.mark.parametrize("V,maxlen,R,B,boost,seed,use_trie", [(12, 6, 100, 2, 2.5, 7, False), (10, 7, 70, 3, 4.0, 11, False), (6, 5, 4, 3, 3.0, 5, True)])
def test_beam_search_table(dev, V, maxlen, R, B, boost, seed, use_trie):
    from gdr_amd import codec
    from oracle import beam_ref, t5_ref
    Vd = V * maxlen + 2
    tab = synth.make_logit_table(B, maxlen, Vd, boost, seed)
    table = torch.from_numpy(tab)
    Td, th = guarded_input(table, tail=torch.full((maxlen * Vd * Vd,), 50.0))                # a query's worth of large logits behind the table
    trie = dtrie = None
    handles = [th]
    if use_trie:
        trie = codec.Trie.from_docids(_docids(V, 2, 3), V)
        ch, chh = guarded_input(torch.from_numpy(trie.child), tail=torch.zeros(64 * V, dtype=torch.int32))     # node ids behind the trie
        eo, eoh = guarded_input(torch.from_numpy(trie.eos_ok), tail=torch.ones(256, dtype=torch.int32))
        struct = _ffi.GdrTrie(ch.data_ptr(), eo.data_ptr(), trie.child.shape[0], int(trie.V))
        dtrie = ops.DeviceTrie(trie, dev)
        handles += [chh, eoh]
    need = lib().gdr_beam_search_table_workspace_bytes(B, R, maxlen, V)
    res = run_guarded(dev, {"ids": ((B * R, maxlen), torch.int64), "len": ((B * R,), torch.int32), "score": ((B * R,), torch.float64)}, need,
                      lambda o, ws, n: lib().gdr_beam_search_table(ptr(Td), B, V, R, maxlen, 0.8, R, C.byref(struct) if use_trie else None,
                                                                   ptr(o["ids"]), ptr(o["len"]), ptr(o["score"]), ptr(ws), n, stream_ptr()),
                      inputs=handles, what="beam_search_table")
    oi, ol, osc = ops.beam_search_table(table.to(dev), V, R, maxlen, 0.8, trie=dtrie)
    assert same_bits(res["ids"], oi) and same_bits(res["len"], ol) and same_bits(res["score"], osc)
    qid = torch.arange(B).repeat_interleave(R)

    def step(seq):
        t = seq.shape[1]
        return table[qid, t - 1, seq[:, -1]] + t5_ref.positional_mask(t, Vd, V)[t - 1]

    if not use_trie:
        ref_dec, ref_sc = beam_ref.beam_search(step, B, R, Vd, maxlen, 0.8)
        dec_ids, sc = ops.finish_generate_output(res["ids"], res["len"], res["score"], maxlen)
        np.testing.assert_allclose(np.array(sc), np.array(ref_sc), rtol=1e-5, atol=1e-5)
        assert np.array_equal(dec_ids.cpu().numpy(), ref_dec.numpy())
    else:                                                            # every returned hypothesis is a docid of the trie (or a prefix cut by EOS)
        body = {tuple(codec.encode_single_newid(s, kary=V)) for s in _docids(V, 2, 3)}
        assert bool(torch.isfinite(res["score"]).any())
        for row, n, sc in zip(res["ids"].cpu().tolist(), res["len"].cpu().tolist(), res["score"].cpu().tolist()):
            if not np.isfinite(sc):
                continue                                             # fewer live hypotheses than beams: the rest is padding
            toks = tuple(t for t in row[1:n] if t > 1)
            assert any(b[:len(toks)] == toks for b in body), row


@covers("gdr_t5_relative_bucket_table")
@pytest.mark.parametrize("bidirectional,qlen,klen", [(1, 1, 1), (1, 40, 40), (0, 7, 129), (1, 128, 128)])
def test_relative_bucket_table_writes_its_host_table_only(bidirectional, qlen, klen):
    """A HOST output: canaries on both sides of the int32[qlen * klen] table; the values against the formula of
    modeling_t5.py:242-288 (oracle/t5_ref.py)."""
    from oracle import t5_ref
    n, pad = qlen * klen, 4096
    buf = (C.c_int32 * (n + 2 * pad))(*([0x5A5A5A5A] * (n + 2 * pad)))
    out = C.cast(C.byref(buf, pad * 4), C.POINTER(C.c_int32))
    assert lib().gdr_t5_relative_bucket_table(bidirectional, 32, 128, qlen, klen, out) == 0
    arr = np.frombuffer(buf, dtype=np.int32)
    assert (arr[:pad] == 0x5A5A5A5A).all() and (arr[pad + n:] == 0x5A5A5A5A).all(), "wrote outside the table"
    rel = torch.arange(klen)[None, :] - torch.arange(qlen)[:, None]
    ref = t5_ref.relative_position_bucket(rel, bidirectional=bool(bidirectional), num_buckets=32, max_distance=128)
    assert np.array_equal(arr[pad:pad + n].reshape(qlen, klen), ref.numpy().astype(np.int32))
    assert torch.equal(ops.relative_bucket_table(bidirectional, 32, 128, qlen, klen), ref.to(torch.int32))
