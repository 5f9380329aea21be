#!/usr/bin/env python3
"""Record tests/golden/g20_linear_f32_forms.npz: what gdr_linear_f32_form(M, N, K, workspace_bytes) of the BUILT library answers
over a fixed grid of shapes and workspace sizes.  Host-only (the reporter launches nothing), needs no GPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_linear_forms.py

The table pins the routing of the fp32 linear (gemm_f32.hip: linear_f32_route) against edits that are meant to leave it alone;
tests/test_abi_memory_host.py asserts that the library reproduces it exactly.  Re-record it only with a change that moves a
threshold on purpose.  The grid straddles every boundary of the ladder:
  * 128x128 tile counts 191 / 192, 256 / 257, 512 / 513 and multiples of 512 (with remainders on both sides of the stream-K
    tail's admission, which also depends on K / 32),
  * M at 1536 / 1537 (small-tile form), K / 32 at 3 / 4, K % 32 != 0, K % 4 != 0 (the reporter's 0),
  * M * lda and N * ldw on both sides of 2^31 elements (the stream-K kernels' 32-bit operand offsets),
  * workspaces of 0, 64 KiB, 1 MiB, the stream-K scratch size - 1, that size, 48 MiB and 112 MiB.
Neither stream-K knob (GDR_GEMM_STREAMK, GDR_GEMM_STREAMK_MID) may be set while recording."""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

KNOBS = ("GDR_GEMM_STREAMK", "GDR_GEMM_STREAMK_MID")
STREAMK_WS_BYTES = 512 * (64 << 10) + 4096

MS = (1, 64, 128, 1536, 1537, 2048, 4096, 12350, 20480, 24448, 24449, 32768, 32769, 65536, 65537, 131072)
NS = (128, 768, 2048, 3072)
KS = (96, 128, 768, 3072, 100, 770)
# one row panel x 191 / 192 and 256 / 257 column tiles; few rows x 15 / 16 column tiles (tiles 180 / 192 at M <= 1536);
# A or W on either side of 2^31 elements; empty and negative shapes
EXTRA = ((64, 24448, 128), (64, 24449, 128), (128, 32768, 768), (128, 32769, 768), (1536, 1920, 768), (1537, 1920, 768),
         (1408, 2176, 768), (1408, 2304, 768),
         (699_000, 128, 3072), (700_001, 128, 3072), (699_050, 128, 3072), (699_051, 128, 3072), (700_001, 3072, 320),
         (700_001, 3072, 64), (640, 699_000, 3072), (640, 700_001, 3072), (66_000, 128, 32_768),
         (0, 768, 768), (-1, 768, 768), (128, 0, 768), (128, 768, 0))
WORKSPACES = (0, 64 << 10, 1 << 20, STREAMK_WS_BYTES - 1, STREAMK_WS_BYTES, 48 << 20, 112 << 20)


def cases():
    shapes = list(itertools.product(MS, NS, KS)) + list(EXTRA)
    return [(m, n, k, ws) for (m, n, k) in shapes for ws in WORKSPACES]


def main():
    assert not any(k in os.environ for k in KNOBS), f"unset {KNOBS} before recording"
    from gdr_amd import _ffi
    l = _ffi.lib()
    assert _ffi.STREAMK_WS_BYTES == STREAMK_WS_BYTES
    rows = np.array([(m, n, k, ws, l.gdr_linear_f32_form(m, n, k, ws)) for (m, n, k, ws) in cases()], dtype=np.int64)
    codes = sorted(set(rows[:, 4].tolist()))
    assert codes == list(range(8)), codes       # 0 and each of the seven GDR_F32_FORM_* codes
    out = os.path.join(HERE, "g20_linear_f32_forms.npz")
    np.savez_compressed(out, cases=rows)
    print(out, rows.shape, {c: int((rows[:, 4] == c).sum()) for c in codes})


if __name__ == "__main__":
    main()
