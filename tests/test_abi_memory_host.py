"""No entry point of include/gdr_hip.h may ship without a guard case: every exported function with a pointer parameter (a device
buffer, or a struct that carries device pointers) must appear in the COVERAGE table of tests/test_gpu_abi_memory.py — filled by
the @covers decorator of the tests that hold it to the memory contract — or in EXEMPT below with its reason.  Needs no GPU."""
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
