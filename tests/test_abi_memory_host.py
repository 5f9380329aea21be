"""No entry point of include/gdr_hip.h may ship without a guard case: every exported function with a pointer parameter (a device
buffer, or a struct that carries device pointers) must appear in the COVERAGE table of tests/test_gpu_abi_memory.py — filled by
the @covers decorator of the tests that hold it to the memory contract — or in EXEMPT below with its reason.  Also the host-only answers that the large-operand tests
(tests/test_gpu_large_offsets.py) rely on: the fp32 linear's route switch at 2^31 elements of A and the refusal of an idx_offset
that would leave int32 doc ids.  Needs no GPU."""
import os
import re

from conftest import REPO

# host-only pointers: nothing here reads or writes device memory
EXEMPT = {
    "gdr_prof_collect": "three HOST arrays of length 8; the opt-in profiler is covered by tests/test_gpu_bench_contract.py",
    "gdr_cluster_key_hash": "host routine over a host token array",
}


def _prototypes():
    text = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:const\s+char\s*\*|int64_t|uint64_t|size_t|int|void)\s+(gdr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        protos[m.group(1)] = " ".join(m.group(2).split())
    return protos


def test_the_parser_sees_the_whole_header():
    from gdr_amd import _ffi
    protos = _prototypes()
    assert set(protos) == set(_ffi.SIGNATURES), set(protos) ^ set(_ffi.SIGNATURES)
    assert "void* workspace" in protos["gdr_sim_topk"] and protos["gdr_abi_version"] == "void"


def test_every_entry_point_with_a_pointer_has_a_guard_case_or_a_reason():
    import test_gpu_abi_memory as gpu
    protos = _prototypes()
    with_pointer = {name for name, params in protos.items() if "*" in params}
    assert len(with_pointer) > 50
    unknown = set(gpu.COVERAGE) - set(protos)
    assert not unknown, f"COVERAGE names functions the header does not declare: {sorted(unknown)}"
    both = set(gpu.COVERAGE) & set(EXEMPT)
    assert not both, f"covered and exempt at once: {sorted(both)}"
    stale = set(EXEMPT) - with_pointer
    assert not stale, f"exemptions for functions that take no pointer (or no longer exist): {sorted(stale)}"
    missing = with_pointer - set(gpu.COVERAGE) - set(EXEMPT)
    assert not missing, ("entry points without a guard case in tests/test_gpu_abi_memory.py (add one, or an exemption with its reason): "
                         f"{sorted(missing)}")
    for name, tests in gpu.COVERAGE.items():
        for t in tests:
            assert callable(getattr(gpu, t, None)), f"COVERAGE[{name}] names {t}, which is not a test of the module"
    # a declaration alone is not a case: outside the @covers lists the name must occur in the module's code (a direct call, or an
    # entry of a form table a test walks), or in the source of the gdr_amd.ops object the module says it reaches it through
    import inspect
    from gdr_amd import ops
    code = re.sub(r"@covers\(.*?\)\n", "", inspect.getsource(gpu), flags=re.S)
    for name in gpu.COVERAGE:
        if name in gpu.VIA_OPS:
            via = gpu.VIA_OPS[name]
            assert name in inspect.getsource(getattr(ops, via)) and f"ops.{via}(" in code, f"{name} is not reached through ops.{via}"
        else:
            assert re.search(r"\b" + name + r"\b", code), f"COVERAGE lists {name}, but no test code names it"
    assert all(len(r.split()) >= 4 for r in EXEMPT.values()), "every exemption states its reason"
    assert len(EXEMPT) <= 4, "the exemption list is meant to stay short"


def test_linear_f32_leaves_the_stream_k_forms_when_a_crosses_2_31_elements():
    """The stream-K kernels keep 32-bit element offsets into A and W (gemm_f32.hip streamk_fits): (M, 128, 3072) takes the
    stream-K tail while M * K < 0x7fffffff and the persistent whole-tile kernel from there on, scratch or not."""
    from gdr_amd import _ffi
    l = _ffi.lib()
    streamk_bytes, tail, persistent = _ffi.STREAMK_WS_BYTES, _ffi.F32_FORM_STREAMK_TAIL, _ffi.F32_FORM_PERSISTENT
    assert 699_000 * 3072 < 0x7fffffff <= 700_001 * 3072
    assert l.gdr_linear_f32_form(699_000, 128, 3072, streamk_bytes) == tail
    assert l.gdr_linear_f32_form(700_001, 128, 3072, streamk_bytes) == persistent
    assert l.gdr_linear_f32_form(699_000, 128, 3072, 0) == persistent and l.gdr_linear_f32_form(700_001, 128, 3072, 0) == persistent
    # the switch sits at the element count, not at a row count: the last M below it and the first M at it
    m_last = (0x7fffffff - 1) // 3072
    assert m_last * 3072 < 0x7fffffff <= (m_last + 1) * 3072
    forms = [l.gdr_linear_f32_form(m, 128, 3072, streamk_bytes) for m in (m_last, m_last + 1)]
    assert forms[1] == persistent and forms[0] in (tail, persistent), forms       # below: whichever the tile count asks for
    # a large C with a small A stays eligible (the epilogue's arithmetic is 64-bit): (700 001, 3072, 320) takes the tail
    assert l.gdr_linear_f32_form(700_001, 3072, 320, streamk_bytes) == tail and l.gdr_linear_f32_form(700_001, 3072, 64, streamk_bytes) == persistent


def test_linear_f32_routing_reproduces_the_recorded_table():
    """gdr_linear_f32_form over the grid of tests/golden/make_golden_linear_forms.py (tile counts around 192 / 256 / 512 and
    multiples of 512, M around 1536, K / 32 around 4, K tails, operands around 2^31 elements, seven workspace sizes) answers
    exactly what the library answered when the table was recorded: an edit that is meant to leave the routing alone leaves
    every one of the 2 835 answers alone.  The stream-K knobs move thresholds, so the test refuses to run with one set."""
    import pytest
    from conftest import golden
    from gdr_amd import _ffi
    knobs = [k for k in ("GDR_GEMM_STREAMK", "GDR_GEMM_STREAMK_MID") if k in os.environ]
    if knobs:
        pytest.fail(f"{knobs} set in the environment: the recorded routing table holds for the default thresholds only; unset and rerun")
    table = golden("g20_linear_f32_forms")["cases"]
    assert table.shape[1] == 5 and table.shape[0] >= 2000
    l = _ffi.lib()
    codes = {getattr(_ffi, n) for n in dir(_ffi) if n.startswith("F32_FORM_")}
    assert len(codes) == 7 and set(table[:, 4].tolist()) == codes | {0}, "every form code and 0 occur in the table"
    wrong = [(m, n, k, ws, want, got) for m, n, k, ws, want in table.tolist()
             for got in [l.gdr_linear_f32_form(m, n, k, ws)] if got != want]
    assert not wrong, f"{len(wrong)} of {len(table)} shapes route differently; (M, N, K, workspace, recorded, now): {wrong[:10]}"


def test_sim_topk_refuses_an_idx_offset_that_leaves_int32_before_any_launch():
    """ids are row + idx_offset in int32: idx_offset + N > 2^31 - 1 is GDR_EINVAL with a message, in all three entry points,
    before anything is launched (the pointers below are never dereferenced)."""
    import ctypes as C
    from gdr_amd import _ffi
    l = _ffi.lib()
    p, ws = C.c_void_p(256), C.c_void_p(4096)
    N, B, d, k = 70_001, 8, 128, 10
    top = 2 ** 31 - 1 - N                                          # the largest admissible offset: the last id is 2^31 - 2
    nbytes = 1 << 30
    for off in (top + 1, 2 ** 31 - 1):
        for name, call in (
                ("gdr_sim_topk", lambda o: l.gdr_sim_topk(p, B, p, N, d, k, o, p, p, None, 0, ws, nbytes, None)),
                ("gdr_sim_topk_bf16", lambda o: l.gdr_sim_topk_bf16(p, B, p, N, d, k, o, p, p, None, 0, ws, nbytes, None)),
                ("gdr_sim_topk_prefilter", lambda o: l.gdr_sim_topk_prefilter(p, B, p, p, 1.0, N, d, k, o, p, p, None, ws, nbytes, None))):
            assert call(off) == _ffi.GDR_EINVAL, (name, off)
            msg = l.gdr_last_error()
            assert b"idx_offset" in msg and str(off).encode() in msg, (name, msg)
    # the check is on the sum: a corpus of one row admits 2^31 - 2 and no more
    assert l.gdr_sim_topk(p, B, p, 1, d, 1, 2 ** 31 - 1, p, p, None, 0, ws, nbytes, None) == _ffi.GDR_EINVAL
    assert b"idx_offset" in l.gdr_last_error()


def test_the_form_codes_of_the_binding_are_the_header_s():
    from gdr_amd import _ffi
    text = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GDR_F32_FORM_(\w+) (\d+)", text)}
    assert len(codes) == 7 and all(getattr(_ffi, "F32_FORM_" + n) == v for n, v in codes.items()), codes
    assert "33 558 528 bytes" in text and _ffi.STREAMK_WS_BYTES == 33558528 == 512 * (64 << 10) + 4096


def test_prefilter_workspace_is_never_below_the_plain_one_and_grows_with_d():
    """gdr_sim_topk_prefilter_workspace_bytes depends on d beyond the bf16 queries it holds: the candidate list is sized for the
    threshold lowered by 2 eps_q, and eps_q / |q| grows like sqrt(d).  Never less than gdr_sim_topk's list, monotone in d."""
    from gdr_amd import _ffi
    l = _ffi.lib()
    for B, N, k in ((8, 70_001, 10), (40, 2_800_003, 100), (512, 320_000, 100), (2048, 1_000_000, 100), (4, 1000, 10)):
        plain = l.gdr_sim_topk_workspace_bytes(B, N, 768, k, 0)
        sizes = [l.gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k) for d in (8, 64, 128, 256, 512, 768, 1024)]
        extra = [s - (B * d * 2 + 255) // 256 * 256 for s, d in zip(sizes, (8, 64, 128, 256, 512, 768, 1024))]   # without the bf16 queries
        assert all(e >= plain for e in extra), (B, N, k, plain, extra)
        assert all(a <= b for a, b in zip(extra, extra[1:])), (B, N, k, extra)
        assert extra[-1] <= 8 * plain, (B, N, k)                     # a larger list, not an exhaustive one
    assert l.gdr_sim_topk_prefilter_workspace_bytes(40, 2_800_003, 768, 100) > 1.5 * l.gdr_sim_topk_workspace_bytes(40, 2_800_003, 768, 100, 0)
