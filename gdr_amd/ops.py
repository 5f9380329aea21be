"""Thin tensor-level wrappers over the C ABI (include/gdr_hip.h).  Inputs/outputs are torch CUDA tensors used
purely as device buffers; all arithmetic happens in libgdr_hip.so."""
import ctypes as C
import math
import os

import torch

from . import _ffi
from ._ffi import check, lib, ptr, stream_ptr


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _ffi.GdrError("gdr_amd ops need CUDA (ROCm) tensors; there is no CPU path")


def _f32c(t):
    if t.dtype != torch.float32:
        raise _ffi.GdrError(f"expected float32 tensor, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def linear(a, w, epilogue=_ffi.EPI_NONE, bias=None, residual=None, out=None, splitk_ws=None):
    """out[M,N] = epilogue(a[M,K] @ w[N,K].T)  — gdr_linear_f32 (gdr_linear_f32_splitk when a scratch tensor is given)."""
    _need_cuda(a, w, bias, residual)
    K = a.shape[-1]
    a2 = _f32c(a).view(-1, K)
    w = _f32c(w)
    M, N = a2.shape[0], w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    res2 = None
    if residual is not None:
        res2 = _f32c(residual).view(-1, N)
    if splitk_ws is not None:
        check(lib().gdr_linear_f32_splitk(ptr(a2), K, ptr(w), w.shape[1], ptr(out), N, M, N, K, epilogue,
                                          ptr(_f32c(bias)) if bias is not None else None, ptr(res2), N, ptr(splitk_ws),
                                          splitk_ws.numel() * splitk_ws.element_size(), stream_ptr()),
              "gdr_linear_f32_splitk")
        return out.view(*a.shape[:-1], N)
    check(lib().gdr_linear_f32(ptr(a2), K, ptr(w), w.shape[1], ptr(out), N, M, N, K, epilogue,
                               ptr(_f32c(bias)) if bias is not None else None, ptr(res2), N, stream_ptr()),
          "gdr_linear_f32")
    return out.view(*a.shape[:-1], N)


def linear_bf16(a, w, epilogue=_ffi.EPI_NONE, bias=None, residual=None, out=None):
    """out[M,N] fp32 = epilogue(a[M,K] @ w[N,K].T) with bf16 operands (fp32 tensors are rounded on the device first) and
    fp32 accumulate — gdr_linear_bf16, the linear of the C5 precision mode."""
    _need_cuda(a, w, bias, residual)
    a = (a if a.dtype == torch.bfloat16 else to_bf16(a)).contiguous()
    w = (w if w.dtype == torch.bfloat16 else to_bf16(w)).contiguous()
    K = a.shape[-1]
    a2 = a.view(-1, K)
    M, N = a2.shape[0], w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    res2 = _f32c(residual).view(-1, N) if residual is not None else None
    check(lib().gdr_linear_bf16(ptr(a2), K, ptr(w), w.shape[1], ptr(out), N, M, N, K, epilogue,
                                ptr(_f32c(bias)) if bias is not None else None, ptr(res2), N, stream_ptr()),
          "gdr_linear_bf16")
    return out.view(*a.shape[:-1], N)


def split_bf16x3(x, padded=True):
    """fp32 [rows, K] -> bf16 [rows, ld] with ld = gdr_split_row_elems(K) >= 3K (padded=False: exactly 3K), a row = [hi | mid | lo | pad]
    with x = hi + mid + lo to 24 bits — gdr_split_f32_bf16x3."""
    _need_cuda(x)
    x = _f32c(x)
    K = x.shape[-1]
    ld = lib().gdr_split_row_elems(K, 6) if padded else 3 * K
    out = torch.zeros(x.shape[:-1] + (ld,), dtype=torch.bfloat16, device=x.device)
    check(lib().gdr_split_f32_bf16x3(ptr(x), ptr(out), x.numel() // K, K, ld, stream_ptr()), "gdr_split_f32_bf16x3")
    return out


def split_f16x2(x):
    """fp32 [rows, K] -> fp16 [rows, 2K], a row = [hi | lo'] with hi = fp16(x), lo' = fp16((x - hi) * 2^11): 22 bits — gdr_split_f32_f16x2."""
    _need_cuda(x)
    x = _f32c(x)
    K = x.shape[-1]
    ld = lib().gdr_split_row_elems(K, 2)
    out = torch.zeros(x.shape[:-1] + (ld,), dtype=torch.float16, device=x.device)
    check(lib().gdr_split_f32_f16x2(ptr(x), ptr(out), x.numel() // K, K, ld, stream_ptr()), "gdr_split_f32_f16x2")
    return out


def linear_split_bf16(a3, w3, K, epilogue=_ffi.EPI_NONE, bias=None, residual=None, out=None, terms=6):
    """out[M,N] fp32 = epilogue(a @ w.T) with a [M,K], w [N,K] given as three bf16 planes per row (split_bf16x3; rows may be padded
    beyond 3K) — gdr_linear_split_bf16: the six leading products of the 24-bit operands on the bf16 MFMA path, fp32 accumulate.
    Exploratory, beside ops.linear."""
    _need_cuda(a3, w3, bias, residual)
    want = torch.float16 if terms == 2 else torch.bfloat16
    planes = 2 if terms == 2 else 3
    if a3.dtype != want or w3.dtype != want or a3.shape[-1] < planes * K or w3.shape[-1] < planes * K:
        raise _ffi.GdrError("linear_split_bf16: operands must be plane rows (bf16 x 3 for terms 6 / 3, fp16 x 2 for terms 2) of the same K")
    a3, w3 = a3.contiguous(), w3.contiguous()
    a2 = a3.view(-1, a3.shape[-1])
    M, N = a2.shape[0], w3.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a3.device)
    res2 = _f32c(residual).view(-1, N) if residual is not None else None
    check(lib().gdr_linear_split_bf16(ptr(a2), a2.shape[1], ptr(w3), w3.shape[1], ptr(out), N, M, N, K, int(terms), epilogue,
                                      ptr(_f32c(bias)) if bias is not None else None, ptr(res2), N, stream_ptr()), "gdr_linear_split_bf16")
    return out.view(*a3.shape[:-1], N)


def l2_normalize(x, eps=1e-12):
    """x / max(||x||_2, eps) over the last dim — gdr_l2_normalize (torch.nn.functional.normalize, dense.py:24-25)."""
    _need_cuda(x)
    x = _f32c(x)
    out = torch.empty_like(x)
    d = x.shape[-1]
    check(lib().gdr_l2_normalize(ptr(x), ptr(out), x.numel() // d, d, float(eps), stream_ptr()), "gdr_l2_normalize")
    return out


def t5_layer_norm(x, weight, eps=1e-6):
    """T5LayerNorm (modeling_t5.py:164-171): weight * (x / sqrt(mean(x^2) + eps)) over the last dim, fp32 — gdr_t5_layer_norm."""
    _need_cuda(x, weight)
    x, weight = _f32c(x), _f32c(weight)
    d = x.shape[-1]
    if weight.numel() != d:
        raise _ffi.GdrError(f"t5_layer_norm: weight has {weight.numel()} elements, rows have {d}")
    out = torch.empty_like(x)
    check(lib().gdr_t5_layer_norm(ptr(x), ptr(weight), ptr(out), x.numel() // d, d, float(eps), stream_ptr()), "gdr_t5_layer_norm")
    return out


class Workspace:
    """Grow-only device scratch (256-byte aligned by the caching allocator), one buffer per HIP stream: calls that are in
    flight on different streams (GDRRetriever.validation_steps, two generate() calls) never share scratch."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, nbytes):
        key = torch.cuda.current_stream(self.device).cuda_stream
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self.bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return buf


def to_bf16(x):
    """fp32 tensor -> bf16 tensor (round-to-nearest-even) — gdr_cast_f32_bf16."""
    _need_cuda(x)
    x = _f32c(x)
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().gdr_cast_f32_bf16(ptr(x), ptr(out), x.numel(), stream_ptr()), "gdr_cast_f32_bf16")
    return out


SIM_TOPK_MAX_K = 8192            # gdr_sim_topk[_bf16], gdr_topk_merge, gdr_topk_pack, gdr_topk_merge_packed: one LDS sort of the list
PREFILTER_MAX_K = 1024           # gdr_sim_topk_prefilter: its one-workgroup tail sorts 4k band keys and rescores them in fp32


class LiveRows:
    """Which rows of a corpus are live, as gdr_sim_topk's GDR_SIM_LIVE_MASK reads it: bit r % 32 of int32 word r // 32 is 1 when
    row r is live.  The words stay on `device` (any torch device: the packing is torch ops), `count` = the number of live rows is
    kept on the host.  set / clear change the words on the device and read back ONE number, how many bits flipped; the words
    themselves are never read back.  New rows (LiveRows(n, device), grow) start dead."""

    def __init__(self, n, device):
        self.n, self.count = int(n), 0
        self._words = torch.zeros(max((self.n + 31) // 32, 1), dtype=torch.int32, device=device)
        self.device = self._words.device

    @property
    def words(self):
        """int32 [ceil(n / 32)]: the bitmap (a view of the backing buffer)."""
        return self._words[:(self.n + 31) // 32]

    @staticmethod
    def _pack(bits):
        """bool [32 W] -> int32 [W]; bit 31 enters as -2^31, so every sum is an int32 value"""
        w = torch.tensor([1 << j for j in range(31)] + [-(1 << 31)], dtype=torch.int64, device=bits.device)
        return (bits.view(-1, 32).to(torch.int64) * w).sum(1).to(torch.int32)

    @classmethod
    def from_bool(cls, live):
        """live: bool [n] (True = live), on the device the bitmap is to stay on."""
        live = torch.as_tensor(live).to(torch.bool).reshape(-1)
        out = cls(live.numel(), live.device)
        if out.n:
            out._words = cls._pack(torch.nn.functional.pad(live, (0, -out.n % 32)))
            out.count = int(live.sum().item())
        return out

    def _flip(self, ids, to):
        ids = torch.as_tensor(ids).reshape(-1).to(torch.int64)
        if ids.numel() == 0:
            return 0
        if int(ids.min()) < 0 or int(ids.max()) >= self.n:           # where the ids are: no sync for host ids
            raise _ffi.GdrError(f"LiveRows: row ids must lie in [0, {self.n})")
        ids = torch.unique(ids.to(self.device))
        w, b = ids >> 5, ids & 31
        now = (self._words[w].to(torch.int64) >> b) & 1
        ch = now != to                                               # distinct bits, all in the other state: adding them is an OR / AND-NOT
        bit = torch.where(b == 31, torch.full_like(b, -(1 << 31)), torch.ones_like(b) << b).to(torch.int32)
        self._words.index_add_(0, w[ch], bit[ch] if to else -bit[ch])    # int32 wraps: +-2^31 flips bit 31
        n = int(ch.sum().item())
        self.count += n if to else -n
        return n

    def set(self, ids):
        """Rows `ids` become live.  Returns how many were dead."""
        return self._flip(ids, 1)

    def clear(self, ids):
        """Rows `ids` become dead.  Returns how many were live."""
        return self._flip(ids, 0)

    def grow(self, n_new):
        """The corpus now has n_new >= n rows; the new ones are dead until set()."""
        n_new = int(n_new)
        if n_new < self.n:
            raise _ffi.GdrError(f"LiveRows.grow: {n_new} < {self.n} rows")
        need = (n_new + 31) // 32
        if need > self._words.numel():
            buf = torch.zeros(max(need, self._words.numel() * 3 // 2 + 8), dtype=torch.int32, device=self.device)
            buf[:self._words.numel()].copy_(self._words)
            self._words = buf
        self.n = n_new
        return self

    def to_bool(self):
        """bool [n] on the device (tests, debugging)."""
        j = torch.arange(self.n, device=self.device)
        return ((self._words[j >> 5].to(torch.int64) >> (j & 31)) & 1).to(torch.bool)


class QueryRows:
    """Which rows of a corpus each of B queries may be given, as gdr_sim_topk's GDR_SIM_QUERY_MASK reads it: one bitmap per query in
    LiveRows' format, `words` int32 [B, ceil(n / 32)], bit r % 32 of word [q, r // 32] is 1 when row r is allowed for query q.  The
    words stay on `device` (any torch device: everything here is torch ops) and nothing is read back; counts() is a device tensor.
    QueryRows(B, n, device) allows nothing; bits past n in the last word are kept 0 by the constructors and ignored by every reader."""

    def __init__(self, B, n, device):
        self.B, self.n = int(B), int(n)
        self._words = torch.zeros((self.B, max((self.n + 31) // 32, 1)), dtype=torch.int32, device=device)
        self.device = self._words.device

    @property
    def words(self):
        """int32 [B, ceil(n / 32)]: the bitmaps (a view of the backing buffer)."""
        return self._words[:, :(self.n + 31) // 32]

    @classmethod
    def from_bool(cls, allowed):
        """allowed: bool [B, n] (True = row may be returned for that query), on the device the bitmaps are to stay on."""
        allowed = torch.as_tensor(allowed).to(torch.bool)
        if allowed.dim() != 2:
            raise _ffi.GdrError(f"QueryRows.from_bool: a bool [B, n] tensor, not {tuple(allowed.shape)}")
        out = cls(allowed.shape[0], allowed.shape[1], allowed.device)
        if out.B and out.n:
            sh = torch.arange(32, dtype=torch.int32, device=allowed.device)   # 1 << 31 wraps to -2^31: distinct bits, every sum an int32
            for lo in range(0, out.B, 64):                                    # 64 queries at a time bound the int32 [*, 32 W] temporary
                bits = torch.nn.functional.pad(allowed[lo:lo + 64], (0, -out.n % 32)).view(-1, out._words.shape[1], 32)
                out._words[lo:lo + 64] = (bits.to(torch.int32) << sh).sum(-1, dtype=torch.int32)
        return out

    @classmethod
    def _from_ids(cls, ids, n, device, denied):
        ids = list(ids)
        dev = torch.device(device) if device is not None else (torch.as_tensor(ids[0]).device if ids else torch.device("cpu"))
        mask = torch.full((len(ids), int(n)), bool(denied), dtype=torch.bool, device=dev)
        for q, r in enumerate(ids):
            r = torch.as_tensor(r).reshape(-1).to(torch.int64)
            if r.numel() == 0:
                continue
            if int(r.min()) < 0 or int(r.max()) >= n:                    # where the ids are: no sync for host ids
                raise _ffi.GdrError(f"QueryRows: row ids must lie in [0, {int(n)})")
            mask[q, r.to(dev)] = not denied
        return cls.from_bool(mask)

    @classmethod
    def from_allowed(cls, ids, n, device=None):
        """ids: B tensors / lists of row ids in [0, n), query q's allowed rows (repeats are fine); everything else is denied."""
        return cls._from_ids(ids, n, device, False)

    @classmethod
    def from_denied(cls, ids, n, device=None):
        """ids: B tensors / lists of row ids in [0, n), the rows query q must not be given; everything else is allowed."""
        return cls._from_ids(ids, n, device, True)

    def to_bool(self):
        """bool [B, n] on the device (tests, debugging)."""
        j = torch.arange(self.n, device=self.device)
        return ((self._words[:, j >> 5].to(torch.int64) >> (j & 31)) & 1).to(torch.bool)

    def counts(self):
        """int64 [B] on the device: how many rows each query allows (bits past n are not counted).  No read-back."""
        x = self.words.to(torch.int64) & 0xFFFFFFFF
        if self.n % 32 and x.numel():
            x = torch.cat([x[:, :-1], x[:, -1:] & ((1 << (self.n % 32)) - 1)], 1)
        x = x - ((x >> 1) & 0x55555555)
        x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
        x = (x + (x >> 4)) & 0x0F0F0F0F
        return (((x * 0x01010101) >> 24) & 0xFF).sum(1)

    def and_(self, live):
        """In place: a row stays allowed only where `live` (a LiveRows over the same n rows, on this device) has it live."""
        if not isinstance(live, LiveRows) or live.n != self.n or live.device != self.device:
            raise _ffi.GdrError(f"QueryRows.and_: an ops.LiveRows over the same {self.n} rows, on the same device")
        self.words.bitwise_and_(live.words)
        return self

    def rows(self, idx):
        """The QueryRows of the sub-batch idx (a tensor / list of query numbers): a copy."""
        idx = torch.as_tensor(idx, device=self.device).reshape(-1).to(torch.int64)
        out = QueryRows(idx.numel(), self.n, self.device)
        out._words = self._words[idx]
        return out


class RowCompaction:
    """The renumbering that drops the dead rows of a corpus (compact_plan; include/gdr_hip_compact.h): n_old rows -> n_new live rows in
    their old order.  new_id int32[n_old] (device): the new row of an old row, -1 for a dead one; old_id int32[n_new] (device): the
    old row of a new row, ascending; identity: nothing was dead.  An identity plan makes every method a no-op that launches nothing
    (it hands back what it was given)."""

    def __init__(self, n_old, n_new, new_id, old_id):
        self.n_old, self.n_new, self.new_id, self.old_id = int(n_old), int(n_new), new_id, old_id
        self.device = new_id.device
        self._ws = Workspace(self.device)

    @property
    def identity(self):
        return self.n_new == self.n_old

    def _row_bytes(self, what, t):
        _need_cuda(t)
        if t.dim() < 1 or t.shape[0] != self.n_old or not t.is_contiguous() or t.device != self.device:
            raise _ffi.GdrError(f"RowCompaction.rows: {what} must be a contiguous [{self.n_old}, ...] tensor on {self.device}, got "
                                f"{tuple(t.shape)} on {t.device}")
        row_bytes = (t.numel() // max(self.n_old, 1)) * t.element_size()
        if row_bytes == 0 or row_bytes % 4:
            raise _ffi.GdrError(f"RowCompaction.rows: a row of {what} is {row_bytes} bytes; gdr_rows_compact moves multiples of 4 bytes")
        return row_bytes

    def rows(self, t, out=None, chunk_rows=0):
        """Compacts the rows of t (contiguous [n_old, ...], any dtype whose row is a multiple of 4 bytes: fp32 / bf16 embeddings,
        int64 token tables) — gdr_rows_compact.  out=None: in place, returns the view t[:n_new] of the same storage (rows >= n_new
        keep what they held); chunk_rows bounds the bounce buffer (0 = the library default, 64 MiB whatever n_old is).  Otherwise
        writes out[:n_new] (same dtype and row shape, not overlapping t) and returns it."""
        row_bytes = self._row_bytes("t", t)
        if out is not None:
            _need_cuda(out)
            if (out.dtype != t.dtype or out.dim() != t.dim() or out.shape[1:] != t.shape[1:] or out.shape[0] < self.n_new
                    or not out.is_contiguous() or out.device != t.device):
                raise _ffi.GdrError(f"RowCompaction.rows: out must be a contiguous {t.dtype} [>= {self.n_new}, ...] tensor with t's row shape")
            if out.data_ptr() == t.data_ptr():
                out = None
        if self.identity:
            if out is None:
                return t
            out[:self.n_new].copy_(t)                                 # nothing to compact: the rows as they are
            return out[:self.n_new]
        if self.n_new == 0:
            return t[:0] if out is None else out[:0]
        if out is not None:
            check(lib().gdr_rows_compact(ptr(t), ptr(out), self.n_old, row_bytes, ptr(self.old_id), self.n_new, 0, None, 0, stream_ptr()),
                  "gdr_rows_compact")
            return out[:self.n_new]
        chunk = int(chunk_rows)
        if chunk < 0:
            raise _ffi.GdrError(f"RowCompaction.rows: chunk_rows={chunk} must not be negative")
        if chunk == 0:                                                # the library default, not beyond what this table needs
            chunk = max((lib().gdr_rows_compact_workspace_bytes(row_bytes, 0) - 256) // row_bytes, 1)
        chunk = min(chunk, self.n_new)
        ws = self._ws.get(lib().gdr_rows_compact_workspace_bytes(row_bytes, chunk))
        check(lib().gdr_rows_compact(ptr(t), ptr(t), self.n_old, row_bytes, ptr(self.old_id), self.n_new, chunk, ptr(ws), ws.numel(),
                                     stream_ptr()), "gdr_rows_compact")
        return t[:self.n_new]

    def ids(self, t, strict=True):
        """Remaps a tensor of doc ids (int32 or int64, any shape, on the device: stored search results, member lists) —
        gdr_ids_remap: a negative id (the -1 padding of result lists) stays, a live row's id becomes its new one.  An id that was
        dead or out of range raises GdrError (one read-back of the status word); strict=False returns -1 there instead and reads
        nothing back.  Returns a new tensor of t's shape and dtype."""
        _need_cuda(t)
        if t.dtype not in (torch.int32, torch.int64) or t.device != self.device:
            raise _ffi.GdrError(f"RowCompaction.ids: an int32 / int64 tensor on {self.device}, got {t.dtype} on {t.device}")
        if self.identity or self.n_old == 0:
            return t
        flat = t.reshape(-1)
        if t.dtype == torch.int64:                                   # doc ids are int32 values; anything larger is out of range
            flat = torch.where((flat >= 2 ** 31) | (flat < -2 ** 31), torch.full_like(flat, 2 ** 31 - 1), flat)
        src = flat.to(torch.int32).contiguous()
        out = torch.empty_like(src)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        check(lib().gdr_ids_remap(ptr(self.new_id), self.n_old, ptr(src), ptr(out), src.numel(), ptr(status), stream_ptr()), "gdr_ids_remap")
        if strict and int(status.item()):
            raise _ffi.GdrError("RowCompaction.ids: an id names a dead row or lies outside the old corpus "
                                f"[0, {self.n_old}) (strict=False maps such ids to -1)")
        return out.to(t.dtype).view(t.shape)

    def query_rows(self, qr):
        """The QueryRows over the n_new rows that allows query q exactly the (surviving) rows qr allowed it — gdr_rowmask_compact."""
        if not isinstance(qr, QueryRows) or qr.n != self.n_old or qr.device != self.device:
            raise _ffi.GdrError(f"RowCompaction.query_rows: an ops.QueryRows over the {self.n_old} old rows, on {self.device}")
        if self.identity:
            return qr
        out = QueryRows(qr.B, self.n_new, self.device)
        if qr.B and self.n_new:
            win = qr._words if qr._words.is_contiguous() else qr._words.contiguous()
            _need_cuda(win)
            check(lib().gdr_rowmask_compact(ptr(win), win.shape[1], qr.B, self.n_old, ptr(self.old_id), self.n_new, ptr(out._words),
                                            out._words.shape[1], stream_ptr()), "gdr_rowmask_compact")
        return out

    def live_rows(self):
        """The LiveRows of the compacted corpus: all n_new rows live."""
        return LiveRows.from_bool(torch.ones(self.n_new, dtype=torch.bool, device=self.device))


def compact_plan(live, workspace=None):
    """LiveRows (on the GPU) -> RowCompaction — gdr_rows_compact_plan: popcounts, a multi-block scan and ordered placement on the
    device.  Reads back exactly one number, the plan's status word: a LiveRows.count that is not the bitmap's popcount raises
    GdrError."""
    if not isinstance(live, LiveRows):
        raise _ffi.GdrError("compact_plan: an ops.LiveRows")
    _need_cuda(live.words)
    dev, N, n_live = live.device, live.n, live.count
    if N == 0:
        z = torch.empty(0, dtype=torch.int32, device=dev)
        return RowCompaction(0, 0, z, z)
    if not 0 <= n_live <= N:
        raise _ffi.GdrError(f"compact_plan: LiveRows.count = {n_live} for {N} rows")
    new_id = torch.empty(N, dtype=torch.int32, device=dev)
    old_id = torch.empty(n_live, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    words = live.words.contiguous()
    ws = (workspace or Workspace(dev)).get(lib().gdr_rows_compact_plan_workspace_bytes(N))
    check(lib().gdr_rows_compact_plan(ptr(words), N, n_live, ptr(new_id), ptr(old_id) if n_live else None, ptr(status), ptr(ws),
                                      ws.numel(), stream_ptr()), "gdr_rows_compact_plan")
    if int(status.item()):
        raise _ffi.GdrError(f"compact_plan: LiveRows.count = {n_live} is not the number of set bits of the bitmap")
    return RowCompaction(N, n_live, new_id, old_id)


# the workspace layout of a masked call — one per call: with allowed=, live= is ANDed into the per-query bitmaps (_place_bitmaps)
def _mask_flag(live, allowed):
    return _ffi.SIM_QUERY_MASK if allowed is not None else _ffi.SIM_LIVE_MASK if live is not None else 0


def _place_bitmaps(ws, B, live, allowed):
    """Writes the head of a masked call's workspace (stream-ordered): allowed's B bitmaps in slots M bytes apart, live ANDed in — or the
    one bitmap of live.  Nothing without either."""
    if allowed is not None:
        words = allowed.words
        M = (4 * words.shape[1] + 255) // 256 * 256
        slots = ws[:B * M].view(torch.int32).view(B, M // 4)[:, :words.shape[1]]   # the padding up to M is ignored: left as it is
        if live is not None:
            torch.bitwise_and(words, live.words, out=slots)
        else:
            slots.copy_(words)
    elif live is not None:
        words = live.words
        ws[:words.numel() * 4].view(torch.int32).copy_(words)


# (values fp32 [B, k], indices int32 [B, k], status int32 [B]), uninitialised: what every top-k entry point fills
def _topk_out(B, k, device):
    return (torch.empty((B, k), dtype=torch.float32, device=device), torch.empty((B, k), dtype=torch.int32, device=device),
            torch.empty((B,), dtype=torch.int32, device=device))


def _sim_topk_raw(Q, D, k, idx_offset, workspace, flags, live=None, allowed=None):
    B, d = Q.shape
    N = D.shape[0]
    flags |= _mask_flag(live, allowed)
    need = lib().gdr_sim_topk_workspace_bytes(B, N, d, k, flags)
    ws = (workspace or Workspace(Q.device)).get(need)
    _place_bitmaps(ws, B, live, allowed)
    vals, idx, status = _topk_out(B, k, Q.device)
    fn = lib().gdr_sim_topk_bf16 if Q.dtype == torch.bfloat16 else lib().gdr_sim_topk
    check(fn(ptr(Q), B, ptr(D), N, d, k, idx_offset, ptr(vals), ptr(idx), ptr(status), flags, ptr(ws), ws.numel(),
             stream_ptr()), "gdr_sim_topk")
    return vals, idx, status


GATHER_MAX_ROWS = 32768          # gather="auto": a query that allows at most this many rows goes to the gather mode (SIM_ROW_GATHER).  Measured
                                 # (tools/bench_query_gather.py; N = 320 000, d = 768, k = 100): the largest count at which the
                                 # gather call beats the dense masked call with its exhaustive re-run at 512 and 32 queries, fp32 and bf16
                                 # (at 65 536 rows the 512-query calls lose)
GATHER_CHUNK_ROWS = 4096         # GDR_SIM_GATHER_CHUNKS counts list capacity in chunks of this many rows
GATHER_MAX_CHUNKS = 256
GATHER_ONE_SORT_ROWS = 8192      # up to two chunks one LDS sort ranks the list (any k); longer lists take chunks + merge rounds, k <= 1024
GATHER_CHUNKED_MAX_K = 1024


def gather_chunks(rows):
    """The chunk field for a per-query capacity of `rows` rows: ceil(rows / 4096), at least 1."""
    return max(1, -(-int(rows) // GATHER_CHUNK_ROWS))


def gather_route(counts, k, max_rows):
    """Which queries of a filtered call go to the gather mode.  counts: how many rows each query's bitmap allows (host ints, after
    the AND with live=).  Returns (narrow query indices, chunks): the queries with count <= max_rows, in order, and the chunk field
    that holds the largest of their counts (0 when there is none).  A list of more than 8192 rows is ranked by chunks + merge
    rounds, which stop at k = 1024: such a query stays on the dense route when k is larger.  Host only."""
    counts = [int(c) for c in counts]
    limit = min(int(max_rows), GATHER_CHUNK_ROWS * GATHER_MAX_CHUNKS)
    if k > GATHER_CHUNKED_MAX_K:
        limit = min(limit, GATHER_ONE_SORT_ROWS)
    narrow = [q for q, c in enumerate(counts) if c <= limit]
    return narrow, (gather_chunks(max(counts[q] for q in narrow)) if narrow else 0)


def _sim_topk_exact(Q, D, k, idx_offset, status, vals, idx, flags, live, allowed):
    """exact_on_overflow: reads the status back (one sync) and re-runs the flagged queries exhaustively, in place.  Returns the status."""
    bad = torch.nonzero(status).flatten()
    _ffi.check_device_fault("sim_topk")                              # nonzero() synchronised
    if bad.numel():
        for lo in range(0, bad.numel(), 64):                     # bounded workspace: 64 queries * N * 8 B
            rows = bad[lo:lo + 64]
            v2, i2, _ = _sim_topk_raw(Q[rows].contiguous(), D, k, idx_offset, None,
                                      _ffi.SIM_EXHAUSTIVE | (flags & _ffi.SIM_NO_STREAM), live,   # the core the caller chose
                                      allowed.rows(rows) if allowed is not None else None)
            vals[rows], idx[rows] = v2, i2
        status = torch.zeros_like(status)
    return status


# sim_topk's three routes.  Each makes its library calls and returns (vals, idx, status); P is the PrefilteredCorpus where sim_topk chose
# the pre-filter (prefilter_route), else None.
# The dense call over every row — the one place that chooses between the (masked) pre-filter over P and the plain entry point:
def _sim_topk_dense(Q, D, P, k, idx_offset, workspace, flags, live, allowed):
    if P is not None:
        return _sim_topk_prefilter_raw(Q, P, k, idx_offset, workspace, live, allowed)
    return _sim_topk_raw(Q, D, k, idx_offset, workspace, flags, live, allowed)


# every query through the gather mode at a capacity of `chunks` chunks, no read-back:
def _sim_topk_gather(Q, D, k, idx_offset, workspace, flags, live, allowed, chunks):
    gflags = (flags & _ffi.SIM_NO_STREAM) | _ffi.SIM_ROW_GATHER | _ffi.sim_gather_chunks(chunks)
    return _sim_topk_raw(Q, D, k, idx_offset, workspace, gflags, live, allowed)


def _sim_topk_auto(Q, D, P, k, idx_offset, workspace, flags, live, allowed):
    """gather="auto": reads the counts back (the one extra sync), sends the narrow queries to ONE gather call and the wide rest to the
    dense call, whose overflows it re-runs here — the result is exact as returned, status all 0.  None when no query is narrow: the
    dense route serves the batch, as without gather=."""
    eff = allowed if live is None else allowed.rows(torch.arange(allowed.B, device=allowed.device)).and_(live)   # a copy: the caller's stays
    narrow, chunks = gather_route(eff.counts().tolist(), k, GATHER_MAX_ROWS)     # the one extra sync
    if not narrow:
        return None
    B = Q.shape[0]
    if len(narrow) == B:
        return _sim_topk_gather(Q, D, k, idx_offset, workspace, flags, None, eff, chunks)   # the capacity holds every count: status is 0
    wide = sorted(set(range(B)) - set(narrow))
    nt, wt = (torch.tensor(x, dtype=torch.int64, device=Q.device) for x in (narrow, wide))
    vals, idx, status = _topk_out(B, k, Q.device)
    status.zero_()
    vals[nt], idx[nt], _ = _sim_topk_gather(Q[nt].contiguous(), D, k, idx_offset, workspace, flags, None, eff.rows(nt), chunks)
    Qw, aw = Q[wt].contiguous(), eff.rows(wt)
    v2, i2, s2 = _sim_topk_dense(Qw, D, P, k, idx_offset, workspace, flags, None, aw)   # masks=True: the wide remainder through the bf16 pre-filter
    _sim_topk_exact(Qw, D, k, idx_offset, s2, v2, i2, flags, None, aw)
    vals[wt], idx[wt] = v2, i2
    return vals, idx, status


def sim_topk(Q, D, k, idx_offset=0, workspace=None, return_status=False, exact_on_overflow=True, flags=0, live=None, allowed=None,
             gather=None):
    """Fused Q·Dᵀ + per-row top-k — gdr_sim_topk.  Returns (values fp32[B,k], indices int32[B,k]), 1 <= k <= min(SIM_TOPK_MAX_K, N).
    D may be an fp32 or bf16 tensor, or a PrefilteredCorpus: the pre-filter serves k <= PREFILTER_MAX_K, a deeper list is the
    plain fp32 call over its rows (the same answer: both return the top-k of the fp32 scores for every input).
    The scratch grows with k (gdr_sim_topk_workspace_bytes; at N = 320 000: 0.7 MiB per query at k = 1024, 2.0 MiB at k = 8192).
    exact_on_overflow=True (the default) reads the per-query status back (one host sync per call) and recomputes any
    query whose candidate list overflowed (degenerate corpora with tens of thousands of tied docs) exhaustively, so the
    result is exact for every input.  Latency-critical callers pass exact_on_overflow=False, return_status=True: no sync,
    and the device status tensor (1 = that row is the top-k of a subset) is theirs to act on.  flags: _ffi.SIM_* bits.
    live: a LiveRows over the N rows of D — the top-k over its live rows only (GDR_SIM_LIVE_MASK; k <= live.count): the list the
    call would return for the matrix of the live rows, with their ids in D.  A PrefilteredCorpus is then searched on the plain fp32
    path — unless it was built with masks=True: then the masked pre-filter serves the call (gdr_sim_topk_prefilter_masked; the same
    answer, see PrefilteredCorpus) —, and the overflow re-run carries the mask.
    allowed: a QueryRows (allowed.B == B, allowed.n == N, on D's device) — row q is the top-k over the rows query q's own bitmap
    allows (GDR_SIM_QUERY_MASK): a filter per query in ONE call.  With live= as well the two are ANDed on their way into the
    workspace, so a dead row never returns whatever the filter says.  How many rows a query allows is known on the device only,
    so nothing raises for a short one: a row with fewer than k allowed (and live) documents ends in -inf / -1.  A PrefilteredCorpus
    is searched on the plain fp32 path, as for live= (masks=True: the masked pre-filter, which with gather="auto" takes the wide
    remainder of the batch only).  A query whose filter keeps a small fraction of the rows overflows its
    candidate list (include/gdr_hip.h, NARROW FILTERS) and is re-run exhaustively with its bitmap — unless the gather mode takes it:
    gather (with allowed=; GDR_SIM_ROW_GATHER): how narrow filters are served.
      None / False  the dense masked call and its exhaustive re-run, launch for launch what the call did before the mode existed.
      an int rows   every query goes through the gather mode with a capacity of ceil(rows / 4096) chunks: only the rows a bitmap
                    allows are scored.  No read-back, so it is usable with exact_on_overflow=False; status[q] = 1 where query q allows
                    more rows than the capacity (exact_on_overflow=True re-runs those exhaustively, as any overflow).
      "auto"        (needs exact_on_overflow=True, which synchronises anyway; otherwise it is False) reads back the per-query counts
                    of the bitmaps as they will be used — after the AND with live= — one more sync, before the launches.  Queries
                    that allow at most GATHER_MAX_ROWS rows (gather_route) go to ONE gather call sized for the largest of them, the
                    rest to the dense masked call as before; an all-narrow batch launches no dense pass.
    DenseModel.search and GDRRetriever.search pass "auto" by default; here the default is None, so that a direct caller's lists stay
    bit for bit the dense call's (the gather pass sums a row in another order than the GEMM core)."""
    P = None
    if isinstance(D, PrefilteredCorpus):
        P, D = D, D.D
        if not prefilter_route(Q.shape[0], D.shape[1], k, flags, P.dnorm_max, live is not None or allowed is not None, P.masks):
            P = None
    _need_cuda(Q, D)
    if D.dtype == torch.bfloat16:                                    # bf16 corpus: queries are cast on the device
        Q = (Q if Q.dtype == torch.bfloat16 else to_bf16(Q)).contiguous()
        D = D.contiguous()
    else:
        Q, D = _f32c(Q), _f32c(D)
    if D.shape[1] != Q.shape[1]:
        raise _ffi.GdrError(f"sim_topk: dim mismatch {Q.shape} vs {D.shape}")
    if k > D.shape[0]:
        raise RuntimeError("selected index k out of range")          # torch.topk's message
    if live is not None:
        if not isinstance(live, LiveRows) or live.n != D.shape[0] or live.device != D.device:
            raise _ffi.GdrError(f"sim_topk: live must be an ops.LiveRows over the {D.shape[0]} rows of D, on its device")
        if k > live.count and allowed is None:
            raise RuntimeError("selected index k out of range")      # as torch.topk over the live rows would
    if allowed is not None:
        if not isinstance(allowed, QueryRows) or allowed.B != Q.shape[0] or allowed.n != D.shape[0] or allowed.device != D.device:
            raise _ffi.GdrError(f"sim_topk: allowed must be an ops.QueryRows of {Q.shape[0]} queries over the {D.shape[0]} rows of D, on its device")
    if gather is None or gather is False or (isinstance(gather, str) and gather == "auto" and (allowed is None or not exact_on_overflow)):
        gather = None
    elif allowed is None or (flags & _ffi.SIM_EXHAUSTIVE):
        raise _ffi.GdrError("sim_topk: gather= ranks the rows a QueryRows allows: it needs allowed= and no SIM_EXHAUSTIVE flag")
    elif gather is True or not (gather == "auto" or (isinstance(gather, int) and 1 <= gather <= GATHER_CHUNK_ROWS * GATHER_MAX_CHUNKS)):
        raise _ffi.GdrError(f'sim_topk: gather must be None, False, "auto" or a row capacity in [1, {GATHER_CHUNK_ROWS * GATHER_MAX_CHUNKS}], not {gather!r}')
    out = _sim_topk_auto(Q, D, P, k, idx_offset, workspace, flags, live, allowed) if gather == "auto" else None
    if out is not None:                                              # exact as it stands: its dense part re-ran its own overflows
        vals, idx, status = out
    else:
        if gather is None or gather == "auto":                       # "auto" with no narrow query
            vals, idx, status = _sim_topk_dense(Q, D, P, k, idx_offset, workspace, flags, live, allowed)
        else:
            vals, idx, status = _sim_topk_gather(Q, D, k, idx_offset, workspace, flags, live, allowed, gather_chunks(gather))
        if exact_on_overflow:
            status = _sim_topk_exact(Q, D, k, idx_offset, status, vals, idx, flags, live, allowed)
    return (vals, idx, status) if return_status else (vals, idx)


class PrefilteredCorpus:
    """An fp32 corpus [N,d] with what gdr_sim_topk_prefilter needs beside it: its bf16 image (RNE, +50 % memory) and the largest
    row norm, both made once on the device.  ops.sim_topk(Q, PrefilteredCorpus(D), k) returns the top-k of the FP32 scores (the
    bf16 pass only decides which few hundred docs per query get one: include/gdr_hip.h).
    The image and the norm bound are SNAPSHOTS of D: after any in-place update of D (an index refresh) call refresh() before the
    next search — or update_rows(ids) when only those rows changed —: a stale image can drop docs from the band, a stale norm bound
    can make the band too narrow.  `.D` is the raw fp32 tensor for everything that is not a search (rerank, gathers).  An all-zero
    corpus (dnorm_max = 0) is served by the fp32 path.
    masks=True: ops.sim_topk(Q, P, k, live=... / allowed=...) goes through the masked pre-filter (gdr_sim_topk_prefilter_masked:
    the exact fp32 top-k over the live / allowed rows) wherever the unmasked call would take the pre-filter.  The
    default is False and then a masked call takes the plain fp32 path, launch for launch as before the masked form existed: the
    two paths return the same documents, but the pre-filter's values are the same dot products summed in another order, and the
    bits of the default object's masked lists are pinned (tests/test_gpu_live_search.py, test_gpu_query_mask.py,
    test_gpu_query_gather.py).  So the masked route is chosen here, where the +50 % memory of the image is chosen."""

    def __init__(self, D, masks=False):
        _need_cuda(D)
        self.masks = bool(masks)
        self._norm2 = torch.zeros(1, dtype=torch.float32, device=D.device)
        self._bind(_f32c(D))
        self._D16_buf = torch.empty(self.D.shape, dtype=torch.bfloat16, device=self.D.device)
        self.refresh()

    def _bind(self, D):
        self.D = D
        self.shape, self.dtype, self.device = D.shape, D.dtype, D.device

    @property
    def D16(self):
        """bf16 [N, d]: the image of D (a view of the backing buffer, which rebind() grows geometrically)."""
        return self._D16_buf[:self.D.shape[0]]

    def _read_norm(self):
        self.dnorm_max = float(self._norm2.item()) ** 0.5 * (1.0 + 1e-6)   # the squared norm is itself rounded

    def refresh(self):
        """Re-derive the bf16 image and the largest row norm from the current contents of D (one sync)."""
        check(lib().gdr_cast_f32_bf16(ptr(self.D), ptr(self._D16_buf), self.D.numel(), stream_ptr()), "gdr_cast_f32_bf16")
        check(lib().gdr_row_norm2_max(ptr(self.D), self.D.shape[0], self.D.shape[1], ptr(self._norm2), stream_ptr()), "gdr_row_norm2_max")
        self._read_norm()
        return self

    def update_rows(self, ids):
        """Rows `ids` of D were rewritten: their rows of the image are re-derived (the bits refresh() would give) and dnorm_max is
        raised to their largest norm if that is larger — ONE gdr_prefilter_update_rows call and a 4-byte read-back.  dnorm_max only
        grows until refresh() is called (a bound that is too large costs band width, never exactness).  ids: row ids in [0, N), any
        integer tensor / list, repeats allowed; checked where they are (host ids: no sync; device ids: one more)."""
        ids = torch.as_tensor(ids).reshape(-1)
        if ids.numel() == 0:
            return self
        if ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise _ffi.GdrError(f"PrefilteredCorpus.update_rows: ids must be integers, got {ids.dtype}")
        N, d = self.D.shape
        if int(ids.min()) < 0 or int(ids.max()) >= N:
            raise _ffi.GdrError(f"PrefilteredCorpus.update_rows: row ids must lie in [0, {N})")
        if d % 8:
            return self.refresh()                                    # no image the pre-filter could use: keep the snapshot whole
        rows = ids.to(device=self.D.device, dtype=torch.int32).contiguous()
        check(lib().gdr_prefilter_update_rows(ptr(self.D), ptr(self._D16_buf), d, ptr(rows), rows.numel(), ptr(self._norm2), stream_ptr()),
              "gdr_prefilter_update_rows")
        self._read_norm()
        return self

    def rebind(self, D_new):
        """The corpus grew: D_new is fp32 [N' >= N, d] whose first N rows hold the data D held (GDRRetriever's geometrically grown
        buffer, reallocated or not).  The image keeps its first N rows — its buffer grows geometrically when N' does not fit — and
        rows N .. N'-1 are derived by update_rows."""
        _need_cuda(D_new)
        N, d = self.D.shape
        if D_new.dtype != torch.float32 or D_new.dim() != 2 or D_new.shape[1] != d or D_new.shape[0] < N or D_new.device != self.D.device:
            raise _ffi.GdrError(f"PrefilteredCorpus.rebind: an fp32 [N' >= {N}, {d}] tensor on {self.D.device}, not {D_new.dtype} {tuple(D_new.shape)}")
        D_new = _f32c(D_new)
        N2 = D_new.shape[0]
        if N2 > self._D16_buf.shape[0]:
            buf = torch.empty((max(N2, N + N // 2 + 64), d), dtype=torch.bfloat16, device=self.D.device)
            buf[:N].copy_(self._D16_buf[:N])
            self._D16_buf = buf
        self._bind(D_new)
        if N2 > N:
            self.update_rows(torch.arange(N, N2, dtype=torch.int32, device=self.D.device))
        return self

    def compact(self, plan, D_new):
        """The corpus was compacted through `plan` (a RowCompaction over its N rows): D_new is the fp32 [n_new, d] matrix of the live
        rows.  The image's rows MOVE (RowCompaction.rows, in place in the image's buffer), they are not recomputed: rounding is per
        row, so the image equals a fresh image of D_new bit for bit.  dnorm_max is kept: the largest norm over a superset of the
        rows is still an upper bound, which is all the band needs (include/gdr_hip_prefilter_mask.h)."""
        _need_cuda(D_new)
        N, d = self.D.shape
        if not isinstance(plan, RowCompaction) or plan.n_old != N:
            raise _ffi.GdrError(f"PrefilteredCorpus.compact: a RowCompaction over the corpus' {N} rows")
        if D_new.dtype != torch.float32 or D_new.dim() != 2 or tuple(D_new.shape) != (plan.n_new, d) or D_new.device != self.D.device:
            raise _ffi.GdrError(f"PrefilteredCorpus.compact: an fp32 [{plan.n_new}, {d}] tensor on {self.D.device}, not {D_new.dtype} "
                                f"{tuple(D_new.shape)}")
        self._bind(_f32c(D_new))
        if d % 2:
            return self.refresh()                                    # a bf16 row of odd d is no multiple of 4 bytes (and no image the pre-filter could use)
        plan.rows(self._D16_buf[:N])
        return self


PREFILTER_MIN_BATCH = 1           # the pre-filter serves every batch size: at B <= 32 its corpus-wide pass is the HBM stream over
                                  # the bf16 image (half the bytes of the fp32 stream): 0.205 vs 0.241 ms at B = 1


def prefilter_route(B, d, k, flags, dnorm_max, masked, masks):
    """Whether ops.sim_topk serves a call over a PrefilteredCorpus through the bf16 pre-filter (host only).  The unmasked conditions:
    B >= PREFILTER_MIN_BATCH, d % 8 == 0, d <= 1024, k <= PREFILTER_MAX_K, no SIM_EXHAUSTIVE, dnorm_max > 0 (an all-zero corpus has no
    band: the fp32 path serves it).  masked: the call has live= or allowed=; it takes the (masked) pre-filter only when the corpus
    was built with masks=True."""
    if masked and not masks:
        return False
    return not (B < PREFILTER_MIN_BATCH or d % 8 or d > 1024 or (flags & _ffi.SIM_EXHAUSTIVE) or k > PREFILTER_MAX_K or not dnorm_max > 0.0)


def _sim_topk_prefilter_raw(Q, P, k, idx_offset, workspace, live=None, allowed=None):
    B, d = Q.shape
    N = P.D.shape[0]
    vals, idx, status = _topk_out(B, k, Q.device)
    flags = _mask_flag(live, allowed)
    if not flags:
        need = lib().gdr_sim_topk_prefilter_workspace_bytes(B, N, d, k)
        ws = (workspace or Workspace(Q.device)).get(need)
        check(lib().gdr_sim_topk_prefilter(ptr(Q), B, ptr(P.D), ptr(P.D16), P.dnorm_max, N, d, k, idx_offset, ptr(vals), ptr(idx),
                                           ptr(status), ptr(ws), ws.numel(), stream_ptr()), "gdr_sim_topk_prefilter")
        return vals, idx, status
    need = lib().gdr_sim_topk_prefilter_masked_workspace_bytes(B, N, d, k, flags)
    ws = (workspace or Workspace(Q.device)).get(need)
    _place_bitmaps(ws, B, live, allowed)
    check(lib().gdr_sim_topk_prefilter_masked(ptr(Q), B, ptr(P.D), ptr(P.D16), P.dnorm_max, N, d, k, idx_offset, ptr(vals), ptr(idx),
                                              ptr(status), flags, ptr(ws), ws.numel(), stream_ptr()), "gdr_sim_topk_prefilter_masked")
    return vals, idx, status


def topk_merge(vals, idx):
    """[G,B,k] per-shard lists -> [B,k] — gdr_topk_merge.  k <= SIM_TOPK_MAX_K."""
    _need_cuda(vals, idx)
    vals, idx = _f32c(vals), idx.contiguous()
    G, B, k = vals.shape
    ov = torch.empty((B, k), dtype=torch.float32, device=vals.device)
    oi = torch.empty((B, k), dtype=torch.int32, device=vals.device)
    check(lib().gdr_topk_merge(ptr(vals), ptr(idx), G, B, k, ptr(ov), ptr(oi), stream_ptr()), "gdr_topk_merge")
    return ov, oi


def topk_pack(vals, idx, status=None):
    """(values fp32[B,k], ids int32[B,k][, status int32[B]]) -> int64[B,k+1] wire form — gdr_topk_pack.  k <= SIM_TOPK_MAX_K."""
    _need_cuda(vals, idx, status)
    vals, idx = _f32c(vals), idx.contiguous()
    B, k = vals.shape
    pairs = torch.empty((B, k + 1), dtype=torch.int64, device=vals.device)
    check(lib().gdr_topk_pack(ptr(vals), ptr(idx), ptr(status), B, k, ptr(pairs), stream_ptr()), "gdr_topk_pack")
    return pairs


def topk_merge_packed(pairs, return_status=False):
    """int64[G,B,k+1] per-shard wire lists -> (values [B,k], ids int32 [B,k][, status int32 [B]]) — gdr_topk_merge_packed.
    k <= SIM_TOPK_MAX_K."""
    _need_cuda(pairs)
    pairs = pairs.contiguous()
    G, B, k1 = pairs.shape
    k = k1 - 1
    ov = torch.empty((B, k), dtype=torch.float32, device=pairs.device)
    oi = torch.empty((B, k), dtype=torch.int32, device=pairs.device)
    st = torch.empty((B,), dtype=torch.int32, device=pairs.device) if return_status else None
    check(lib().gdr_topk_merge_packed(ptr(pairs), G, B, k, ptr(ov), ptr(oi), ptr(st), stream_ptr()),
          "gdr_topk_merge_packed")
    return (ov, oi, st) if return_status else (ov, oi)


_RERANK_WS = {}


def rerank_topk(q, D, cand_offsets, cand_ids, beam_scores, alphas, k, func="tanh", max_cand=None, doc_range=None,
                positions=False, workspace=None, cand_stride=0, chunked=False, row_queries=False):
    """In-cluster rerank — gdr_rerank_topk / gdr_rerank_topk_bf16 (chosen by D.dtype; a bf16 corpus is gathered as bf16,
    never up-cast).  Returns (values fp32[B,A,k], doc ids int32[B,A,k]).
    cand_stride=0: cand_offsets int32[B*R+1] is ONE CSR into cand_ids (the reference's concatenation order);
    cand_stride>0: per-query blocks — cand_offsets int32[B,R+1] relative, cand_ids int32[B,cand_stride] (DeviceClusterIndex).
    max_cand: bound of any query's candidate count, at most RERANK_LONG_MAX_CAND; None reads it from the CSR (one host
    sync).  Up to RERANK_MAX_CAND one LDS sort ranks a query's list; above, chunks of RERANK_CHUNK positions are sorted and
    their first k merged (k <= 1024 there) — the same list bit for bit.  chunked=True takes that form at any max_cand
    (GDR_RERANK_CHUNKED: the A/B switch of tests and tools).
    doc_range=(lo, hi): D holds rows [lo, hi) of the corpus, candidates outside are skipped (sharded GDR mode, dist.py);
    positions=True returns candidate positions within the query's list instead of doc ids (what the shard merge needs).
    row_queries=True (GDR_RERANK_ROW_QUERIES): q is fp32[B*R, d], a vector per (query, segment) — a candidate of segment j of
    query b is scored against q[b*R + j] (the decoder-side stage-2 queries); everything else is unchanged."""
    _need_cuda(q, D, cand_offsets, cand_ids, beam_scores)
    q, beam_scores = _f32c(q), _f32c(beam_scores)
    if D.dtype == torch.bfloat16:
        fn, D = lib().gdr_rerank_topk_bf16, D.contiguous()
    else:
        fn, D = lib().gdr_rerank_topk, _f32c(D)
    if D.dim() != 2 or D.shape[1] != q.shape[1]:
        raise _ffi.GdrError(f"rerank_topk: dim mismatch {tuple(q.shape)} vs {tuple(D.shape)}")
    B, R = beam_scores.shape
    if row_queries and (q.dim() != 2 or q.shape[0] != B * R):
        raise _ffi.GdrError(f"rerank_topk: row_queries needs q of B*R = {B * R} rows, got {tuple(q.shape)}")
    al = torch.as_tensor(alphas, dtype=torch.float32, device=q.device)
    A = al.numel()
    if max_cand is None:
        if cand_stride:
            max_cand = int(cand_offsets.view(B, R + 1)[:, R].max().item())
        else:
            o = cand_offsets.view(-1)[::R]
            max_cand = int((o[1:] - o[:-1]).max().item())
    max_cand = max(int(max_cand), 1)
    if cand_stride and cand_stride < max_cand:
        raise _ffi.GdrError(f"rerank_topk: cand_stride {cand_stride} < max_cand {max_cand}")
    lo, hi = (0, D.shape[0]) if doc_range is None else (int(doc_range[0]), int(doc_range[1]))
    if hi - lo != D.shape[0]:
        raise _ffi.GdrError(f"rerank_topk: doc_range {(lo, hi)} does not match the {D.shape[0]} rows given")
    ws_bytes = lib().gdr_rerank_workspace_bytes(B, max(max_cand, RERANK_MAX_CAND + 1) if chunked else max_cand)
    ws = (workspace or _RERANK_WS.setdefault(q.device, Workspace(q.device))).get(ws_bytes)
    ov = torch.empty((B, A, k), dtype=torch.float32, device=q.device)
    oi = torch.empty((B, A, k), dtype=torch.int32, device=q.device)
    check(fn(ptr(q), ptr(D), q.shape[1], ptr(cand_offsets), ptr(cand_ids), ptr(beam_scores), B, R, ptr(al), A, k,
             0 if func == "tanh" else 1, ptr(ov), ptr(oi), max_cand, int(cand_stride), lo, hi,
             (_ffi.RERANK_POSITIONS if positions else 0) | (_ffi.RERANK_CHUNKED if chunked else 0) |
             (_ffi.RERANK_ROW_QUERIES if row_queries else 0),
             ptr(ws), ws.numel(), stream_ptr()), "gdr_rerank_topk")
    return ov, oi


def rerank_wire_pack(q, beam_scores, cand_offsets, cand_ids):
    """(q fp32[B,d], beam fp32[B,R], offsets int32[B,R+1], ids int32[B,stride]) -> int32[B, d+2R+1+stride], the exchange row
    of the sharded in-cluster rerank — gdr_rerank_wire_pack."""
    _need_cuda(q, beam_scores, cand_offsets, cand_ids)
    q, beam_scores = _f32c(q), _f32c(beam_scores)
    cand_offsets, cand_ids = cand_offsets.to(torch.int32).contiguous(), cand_ids.to(torch.int32).contiguous()
    (B, d), R, stride = q.shape, beam_scores.shape[1], cand_ids.shape[1]
    wire = torch.empty((B, d + 2 * R + 1 + stride), dtype=torch.int32, device=q.device)
    check(lib().gdr_rerank_wire_pack(ptr(q), ptr(beam_scores), ptr(cand_offsets), ptr(cand_ids), B, d, R, stride, ptr(wire),
                                     stream_ptr()), "gdr_rerank_wire_pack")
    return wire


def rerank_wire_unpack(wire, d, R, stride):
    """int32[B, d+2R+1+stride] -> (q fp32[B,d], beam fp32[B,R], offsets int32[B,R+1], ids int32[B,stride]) — gdr_rerank_wire_unpack."""
    _need_cuda(wire)
    wire = wire.contiguous()
    B = wire.shape[0]
    if wire.dtype != torch.int32 or wire.shape[1] != d + 2 * R + 1 + stride:
        raise _ffi.GdrError(f"rerank_wire_unpack: wire {tuple(wire.shape)} {wire.dtype} does not match d={d} R={R} stride={stride}")
    q = torch.empty((B, d), dtype=torch.float32, device=wire.device)
    beam = torch.empty((B, R), dtype=torch.float32, device=wire.device)
    offs = torch.empty((B, R + 1), dtype=torch.int32, device=wire.device)
    ids = torch.empty((B, stride), dtype=torch.int32, device=wire.device)
    check(lib().gdr_rerank_wire_unpack(ptr(wire), B, d, R, stride, ptr(q), ptr(beam), ptr(offs), ptr(ids), stream_ptr()),
          "gdr_rerank_wire_unpack")
    return q, beam, offs, ids


def rerank_positions_to_ids(pos, cand_ids):
    """pos int32[B, ...] candidate positions (merged GDR_RERANK_POSITIONS lists; < 0 = padding) -> doc ids int32 of the same
    shape through cand_ids int32[B, stride] — gdr_rerank_positions_to_ids."""
    _need_cuda(pos, cand_ids)
    pos, cand_ids = pos.to(torch.int32).contiguous(), cand_ids.to(torch.int32).contiguous()
    B, stride = cand_ids.shape
    out = torch.empty_like(pos)
    check(lib().gdr_rerank_positions_to_ids(ptr(pos), ptr(cand_ids), B, pos.numel() // B, stride, ptr(out), stream_ptr()),
          "gdr_rerank_positions_to_ids")
    return out


RERANK_MAX_CAND = 8192          # csrc/rerank.hip RR_MAX_CAND: the LDS sort of one (alpha, query) list
RERANK_LONG_MAX_CAND = 1 << 20  # RR_LONG_MAX_CAND: longer lists are sorted in chunks whose first k are merged
RERANK_CHUNK = 4096             # RR_LCH: candidate positions per chunk of the long-list select


def block_max_cand(cand_offsets, R, stride, cap=RERANK_MAX_CAND):
    """The `max_cand` to hand gdr_rerank_topk for candidate blocks of width `stride` = num beams x LARGEST cluster of the
    corpus.  While that worst case fits ONE LDS sort (8192) it is used as is — nothing synchronises.  Beyond that the bound
    comes from the data (one read-back of the per-query counts, this case only): one outlier cluster must not push every
    step to the long-list form, or fail it, when the clusters actually decoded are small.  Only a query that REALLY has more
    than `cap` candidates is refused: cap=RERANK_LONG_MAX_CAND is what the rerank accepts (the retriever passes it); the
    default keeps a caller on the one-sort form and refuses above 8192, as the host CSR path once did."""
    if stride <= RERANK_MAX_CAND:
        return max(int(stride), 1)
    real = int(cand_offsets.view(-1, R + 1)[:, R].max().item())
    if real > cap:
        raise _ffi.GdrError(f"rerank: a query decoded {real} candidate docs; the in-cluster rerank ranks at most "
                            f"{cap} per query")
    return max(real, 1)


class DeviceClusterIndex:
    """codec.ClusterIndex resident on the GPU (include/gdr_hip.h GdrClusterIndex): the clusters' token bodies in an
    exact-match hash table + the member CSR, so that gdr_cluster_candidates turns generate()'s output rows into the rerank's
    candidate CSR without a host round trip (main_models.py:1398,1441-1443)."""

    def __init__(self, index, device, V, position=1, kary=30):
        import numpy as np
        bodies = index.token_bodies(V, position=position, kary=kary)       # list of int lists, None = unreachable name
        n = len(index.names)
        key_len = max([len(b) for b in bodies if b is not None] + [1])
        keys = np.full((max(n, 1), key_len), -1, np.int32)
        lens = np.full(max(n, 1), -1, np.int32)
        T = 4
        while T < 2 * max(n, 1):
            T <<= 1
        slots = np.full(T, -1, np.int32)
        hfn = lib().gdr_cluster_key_hash
        where = {}
        for c, b in enumerate(bodies):
            if b is None:
                continue
            where[tuple(b)] = c                                            # a repeated name: the last one wins, like the dict
        for b, c in where.items():
            keys[c, :len(b)] = b
            lens[c] = len(b)
            arr = (C.c_int32 * max(len(b), 1))(*b)
            slot = int(hfn(arr, len(b))) & (T - 1)
            while slots[slot] >= 0:
                slot = (slot + 1) & (T - 1)
            slots[slot] = c
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
        self.slots, self.keys, self.lens = dev(slots), dev(keys), dev(lens)
        self.offsets, self.members = dev(index.offsets.astype(np.int32)), dev(index.members.astype(np.int32) if index.members.size
                                                                             else np.zeros(1, np.int32))
        self.max_cluster = int(np.diff(index.offsets).max()) if n else 0
        self.n_members = int(index.members.size)
        self.key_len, self.table_size = key_len, T
        self._make_struct()

    def _make_struct(self):
        self.struct = _ffi.GdrClusterIndex(self.offsets.numel() - 1, self.key_len, self.table_size, self.slots.data_ptr(),
                                           self.keys.data_ptr(), self.lens.data_ptr(), self.offsets.data_ptr(),
                                           self.members.data_ptr())

    def insert(self, new_ids, new_cluster, target_map=None, streams=()):
        """Merges documents into the member CSR on the device (cluster_insert): every cluster keeps its members in order,
        followed by the ids it received in ascending order.  new_ids int32[n] ascending, new_cluster int32[n] cluster indices
        (or indices into target_map int32, the compact -> cluster map of FrozenCentroids).  Swaps in the merged CSR, updates
        max_cluster (one read-back) and rebuilds `struct` (it holds raw pointers).  The old arrays are kept alive on every
        stream in `streams` (record_stream): a step enqueued there before this call may still read them."""
        offs, mem, mx = cluster_insert(self.offsets, self.members[:self.n_members], new_ids, new_cluster, target_map)
        for t in (self.offsets, self.members):
            for st in streams:
                t.record_stream(st)
        self.offsets, self.members = offs, (mem if mem.numel() else torch.zeros(1, dtype=torch.int32, device=mem.device))
        self.n_members, self.max_cluster = int(mem.numel()), mx
        self._make_struct()

    def remove(self, ids, streams=()):
        """Takes documents out of the member CSR on the device (cluster_remove): ids int32[n] strictly ascending; every cluster
        keeps its surviving members in their order, an id that is in no cluster is ignored.  Swaps in the compacted CSR, updates
        n_members and max_cluster (which may shrink, and with it the candidate stride of candidates()) and rebuilds `struct`;
        the old arrays are kept alive on every stream in `streams`, as in insert().  Returns the number of ids removed."""
        offs, mem, mx, gone = cluster_remove(self.offsets, self.members[:self.n_members], ids)
        for t in (self.offsets, self.members):
            for st in streams:
                t.record_stream(st)
        self.offsets, self.members = offs, (mem if mem.numel() else torch.zeros(1, dtype=torch.int32, device=mem.device))
        self.n_members, self.max_cluster = int(mem.numel()), mx
        self._make_struct()
        return gone

    def compact(self, plan):
        """The corpus was compacted through `plan` (a RowCompaction): every member becomes its new id, in place in the device member
        list (gdr_ids_remap); the offsets are untouched — the map is monotone, so every cluster keeps its members in their order.
        A member that names a dead or unknown row raises GdrError (one read-back) and leaves the list as it was."""
        if not isinstance(plan, RowCompaction):
            raise _ffi.GdrError("DeviceClusterIndex.compact: an ops.RowCompaction")
        if plan.identity or self.n_members == 0:
            return
        try:
            mem = plan.ids(self.members[:self.n_members])
        except _ffi.GdrError as e:
            raise _ffi.GdrError(f"DeviceClusterIndex.compact: a cluster member is not a live row of the plan ({e})") from None
        self.members[:self.n_members].copy_(mem)

    def candidates(self, out_ids, B, R):
        """out_ids int64[B*R, max_length] (device, untrimmed) -> (cluster_of int32[B*R], cand_offsets int32[B,R+1],
        cand_ids int32[B,stride], stride = R * largest cluster) — the per-query block layout of rerank_topk
        (cand_stride=stride, max_cand=stride); all on the device, nothing synchronises."""
        _need_cuda(out_ids)
        out_ids = out_ids.contiguous()
        stride = max(R * self.max_cluster, 1)
        cl = torch.empty((B * R,), dtype=torch.int32, device=out_ids.device)
        offs = torch.empty((B, R + 1), dtype=torch.int32, device=out_ids.device)
        ids = torch.empty((B, stride), dtype=torch.int32, device=out_ids.device)
        check(lib().gdr_cluster_candidates(C.byref(self.struct), ptr(out_ids), B, R, out_ids.shape[1], ptr(cl), ptr(offs),
                                           ptr(ids), stride, stream_ptr()), "gdr_cluster_candidates")
        return cl, offs, ids, stride


def cluster_centroids(D, index):
    """(centroids fp32[C,d], counts int32[C]) of the clusters of `index` (codec.ClusterIndex) over D fp32[N,d] —
    gdr_cluster_centroids.  Each centroid is the mean of its members' rows, bit-identical to the reference's
    tree_embedding_calculate (main_models.py:154-179): the members are put in ascending order here, once, on the host (index
    preparation), and the device adds them in that order.  An empty cluster has count 0 and a zero row."""
    import numpy as np
    _need_cuda(D)
    D = _f32c(D)
    N, d = D.shape
    C_ = len(index.names)
    if C_ == 0:
        raise _ffi.GdrError("cluster_centroids: the index has no clusters")
    mem = index.sorted_members()
    if mem.size and (int(mem.min()) < 0 or int(mem.max()) >= N):
        raise _ffi.GdrError(f"cluster_centroids: member ids outside [0, {N})")
    offs = torch.from_numpy(np.ascontiguousarray(index.offsets, dtype=np.int32)).to(D.device)
    mem_d = torch.from_numpy(mem if mem.size else np.zeros(1, np.int32)).to(D.device)
    cent = torch.empty((C_, d), dtype=torch.float32, device=D.device)
    counts = torch.empty((C_,), dtype=torch.int32, device=D.device)
    check(lib().gdr_cluster_centroids(ptr(D), N, d, ptr(offs), ptr(mem_d), int(mem.size), C_, ptr(cent), ptr(counts),
                                      stream_ptr()), "gdr_cluster_centroids")
    return cent, counts


ASSIGN_CHUNK = 4096                # rows per gdr_sim_topk call of the assignment: ~0.5 GB of workspace at 16k centroids


def _nearest_compact(X, compact, chunk=ASSIGN_CHUNK, workspace=None):
    """(compact index int32[n], its fp32 score [n]).  Always the tiled GEMM core (SIM_NO_STREAM): at B <= 32 gdr_sim_topk would
    otherwise take the stream kernel, which sums K in another order — a row's score, and so its cluster near a tie, would
    depend on how many rows were in the call.  The GEMM core has no split-K: every row's bits are the same for any B, so
    adding documents in k calls assigns them as one call does."""
    n = X.shape[0]
    out = torch.empty((n,), dtype=torch.int32, device=X.device)
    val = torch.empty((n,), dtype=torch.float32, device=X.device)
    ws = workspace or Workspace(X.device)
    for lo in range(0, n, chunk):
        v, i = sim_topk(X[lo:lo + chunk], compact, 1, workspace=ws, flags=_ffi.SIM_NO_STREAM)   # exact_on_overflow stays on
        out[lo:lo + chunk], val[lo:lo + chunk] = i[:, 0], v[:, 0]
    return out, val


def nearest_cluster(X, centroids, counts, chunk=ASSIGN_CHUNK):
    """int32[n]: for every row of X fp32[n,d] the cluster whose centroid has the largest fp32 dot product with it, among the
    clusters with counts > 0 (the reference's argmax over the set of clusters that hold documents, main_models.py:268-295).
    Ties: the higher score, then the lower cluster index — gdr_sim_topk with k = 1 over the compacted non-empty centroids,
    in chunks of `chunk` rows (bounded workspace)."""
    fc = FrozenCentroids.from_tensors(centroids, counts)
    return fc.assign(X, chunk=chunk)


class FrozenCentroids:
    """The centroids of an index, computed once (the reference never updates them: insertions do not move a centroid), with
    the compacted matrix of the non-empty ones and its compact -> cluster map."""

    def __init__(self, D=None, index=None):
        if D is not None:
            self._set(*cluster_centroids(D, index))

    @staticmethod
    def from_tensors(centroids, counts):
        fc = FrozenCentroids()
        fc._set(_f32c(centroids), counts)
        return fc

    def _set(self, centroids, counts):
        _need_cuda(centroids, counts)
        self.centroids, self.counts = centroids, counts.to(torch.int32)
        nz = torch.nonzero(self.counts > 0).flatten()
        if nz.numel() == 0:
            raise _ffi.GdrError("no cluster has a member: there is no centroid to assign to")
        self.cmap = nz.to(torch.int32)
        self.compact = centroids.index_select(0, nz).contiguous()

    def assign(self, X, compact=False, chunk=ASSIGN_CHUNK, return_scores=False):
        """Nearest non-empty cluster of every row of X: cluster indices int32[n], or (compact=True) indices into `cmap`;
        with return_scores=True also the winning fp32 scores [n].  A row's result does not depend on the other rows of the call."""
        _need_cuda(X)
        X = _f32c(X)
        if X.dim() != 2 or X.shape[1] != self.compact.shape[1]:
            raise _ffi.GdrError(f"assign: rows {tuple(X.shape)} vs centroids of dim {self.compact.shape[1]}")
        if X.shape[0] == 0:
            ci, val = (torch.empty((0,), dtype=torch.int32, device=X.device),
                       torch.empty((0,), dtype=torch.float32, device=X.device))
        else:
            ci, val = _nearest_compact(X, self.compact, chunk=chunk)
        ci = ci if compact else self.cmap[ci.long()]
        return (ci, val) if return_scores else ci


def cluster_insert(offsets, members, new_ids, new_cluster, target_map=None, workspace=None):
    """gdr_cluster_insert: the member CSR (offsets int32[C+1], members int32[n_old]) + new_ids int32[n] (ascending) with
    their clusters new_cluster int32[n] (or indices into target_map) -> (offsets int32[C+1], members int32[n_old+n], largest
    cluster).  Every cluster keeps its members in order, followed by the ids it received in ascending order.  One read-back:
    the largest cluster size."""
    _need_cuda(offsets, members, new_ids, new_cluster, target_map)
    C_ = offsets.numel() - 1
    n_old, n = members.numel(), new_ids.numel()
    if new_cluster.numel() != n:
        raise _ffi.GdrError(f"cluster_insert: {n} ids but {new_cluster.numel()} targets")
    for t in (offsets, members, new_ids, new_cluster) + ((target_map,) if target_map is not None else ()):
        if t.dtype != torch.int32:
            raise _ffi.GdrError(f"cluster_insert: expected int32, got {t.dtype}")
    offsets, members, new_ids, new_cluster = (t.contiguous() for t in (offsets, members, new_ids, new_cluster))
    dev = offsets.device
    out_off = torch.empty((C_ + 1,), dtype=torch.int32, device=dev)
    out_mem = torch.empty((max(n_old + n, 1),), dtype=torch.int32, device=dev)
    out_max = torch.empty((1,), dtype=torch.int32, device=dev)
    need = lib().gdr_cluster_insert_workspace_bytes(C_)
    ws = (workspace or Workspace(dev)).get(need)
    n_map = target_map.numel() if target_map is not None else 0
    check(lib().gdr_cluster_insert(ptr(offsets), ptr(members) if n_old else None, C_, n_old, ptr(new_ids) if n else None,
                                   ptr(new_cluster) if n else None, n, ptr(target_map) if n_map else None, n_map, ptr(out_off),
                                   ptr(out_mem), ptr(out_max), ptr(ws), ws.numel(), stream_ptr()), "gdr_cluster_insert")
    mx = int(out_max.item())
    if mx < 0:
        raise _ffi.GdrError("cluster_insert: a target is out of range or the old offsets are inconsistent")
    return out_off, out_mem[:n_old + n], mx


def cluster_remove(offsets, members, remove_ids, workspace=None):
    """gdr_cluster_insert in its removal mode (new_target == NULL): the member CSR (offsets int32[C+1], members int32[n_old],
    segments in any order) minus remove_ids int32[n] (STRICTLY ascending; checked here, one read-back) -> (offsets int32[C+1],
    members int32[n_left], largest cluster, number of ids removed).  Every cluster keeps its surviving members in their order;
    an id that is in no cluster is ignored.  One more read-back: the largest cluster size and the new total."""
    for t in (offsets, members, remove_ids):
        if t.dtype != torch.int32:
            raise _ffi.GdrError(f"cluster_remove: expected int32, got {t.dtype}")
    C_ = offsets.numel() - 1
    n_old, n = members.numel(), remove_ids.numel()
    if n > 1 and not bool((remove_ids[1:] > remove_ids[:-1]).all()):
        raise _ffi.GdrError("cluster_remove: remove_ids must be strictly ascending")
    _need_cuda(offsets, members, remove_ids)
    offsets, members, remove_ids = (t.contiguous() for t in (offsets, members, remove_ids))
    dev = offsets.device
    out_off = torch.empty((C_ + 2,), dtype=torch.int32, device=dev)             # [C+1] = out_max: one read-back for both
    out_mem = torch.empty((max(n_old, 1),), dtype=torch.int32, device=dev)
    need = lib().gdr_cluster_insert_workspace_bytes(C_)
    ws = (workspace or Workspace(dev)).get(need)
    check(lib().gdr_cluster_insert(ptr(offsets), ptr(members) if n_old else None, C_, n_old, ptr(remove_ids) if n else None,
                                   None, n, None, 0, ptr(out_off), ptr(out_mem), ptr(out_off[C_ + 1:]), ptr(ws), ws.numel(),
                                   stream_ptr()), "gdr_cluster_insert")
    n_left, mx = (int(x) for x in out_off[C_:].tolist())
    if mx < 0:
        raise _ffi.GdrError("cluster_remove: the old offsets are inconsistent")
    return out_off[:C_ + 1], out_mem[:n_left], mx, n_old - n_left


KMEANS_MAX_K = 64
KMEANS_MAX_D = 4096


def cluster_centroids_csr(D, offsets, members, n_members=None):
    """gdr_cluster_centroids over a member CSR that already lives on the device (offsets int32[C+1], members int32[>= n_members],
    every segment ascending) -> (centroids fp32[C,d], counts int32[C]).  The k-means update step; no validation read-back."""
    _need_cuda(D, offsets, members)
    D = _f32c(D)
    if offsets.dtype != torch.int32 or members.dtype != torch.int32:
        raise _ffi.GdrError("cluster_centroids_csr: expected int32 offsets / members")
    N, d = D.shape
    C_ = offsets.numel() - 1
    n = members.numel() if n_members is None else int(n_members)
    cent = torch.empty((C_, d), dtype=torch.float32, device=D.device)
    counts = torch.empty((C_,), dtype=torch.int32, device=D.device)
    check(lib().gdr_cluster_centroids(ptr(D), N, d, ptr(offsets.contiguous()), ptr(members.contiguous()), n, C_, ptr(cent),
                                      ptr(counts), stream_ptr()), "gdr_cluster_centroids")
    return cent, counts


def kmeans_worklist(node_offsets, tile):
    """work int32[n_work, 2] = (node, first row position) of every `tile`-row tile of every node of the CSR node_offsets
    int32[S+1] (device), nodes and tiles ascending — the list gdr_kmeans_assign / gdr_kmeans_partition walk.  Built in torch;
    one read-back (the number of tiles)."""
    off = node_offsets.to(torch.int64)
    sizes = off[1:] - off[:-1]
    nt = (sizes + (tile - 1)) // tile
    total = int(nt.sum().item())
    S = sizes.numel()
    node = torch.repeat_interleave(torch.arange(S, device=off.device), nt, output_size=total)
    first = torch.cumsum(nt, 0) - nt
    q = torch.arange(total, device=off.device) - first[node]
    return torch.stack([node, off[node] + q * tile], 1).to(torch.int32).contiguous()


def _kmeans_check(what, D, rows, node_offsets, k):
    _need_cuda(D, rows, node_offsets)
    if D is not None:
        if D.dtype != torch.float32:
            raise _ffi.GdrError(f"{what}: the corpus must be float32, got {D.dtype} (a bf16 corpus is not supported)")
        if D.dim() != 2 or D.shape[1] % 4 or not 4 <= D.shape[1] <= KMEANS_MAX_D:
            raise _ffi.GdrError(f"{what}: d={D.shape[-1]} (needs d % 4 == 0, 4 <= d <= {KMEANS_MAX_D})")
        if D.shape[0] >= 1 << 31:
            raise _ffi.GdrError(f"{what}: N={D.shape[0]} does not fit int32 doc ids")
    if not 2 <= int(k) <= KMEANS_MAX_K:
        raise _ffi.GdrError(f"{what}: k={k} (needs 2 <= k <= {KMEANS_MAX_K})")
    for t in (rows, node_offsets):
        if t.dtype != torch.int32:
            raise _ffi.GdrError(f"{what}: expected int32, got {t.dtype}")
    if rows.numel() == 0 or node_offsets.numel() < 2:
        raise _ffi.GdrError(f"{what}: empty level")


def kmeans_assign(D, rows, node_offsets, centroids, k, work=None, prev_labels=None, workspace=None):
    """gdr_kmeans_assign: one Lloyd E-step over the nodes of a level.  D fp32[N,d]; rows int32[n] (doc ids, ascending inside a
    node), node_offsets int32[S+1]; centroids fp32[S*k, d]; work = kmeans_worklist(node_offsets, gdr_kmeans_assign_tile()) (built
    here when absent) -> (labels int32[n], score fp32[n] = x.c - |c|^2/2 of the label, changed int32[S] = labels per node that
    differ from prev_labels, status int32[1]: non-zero when a work item was malformed).  No read-back."""
    _kmeans_check("kmeans_assign", D, rows, node_offsets, k)
    _need_cuda(centroids, work, prev_labels)
    D, centroids = _f32c(D), _f32c(centroids)
    rows, node_offsets = rows.contiguous(), node_offsets.contiguous()
    n, S = rows.numel(), node_offsets.numel() - 1
    if tuple(centroids.shape) != (S * k, D.shape[1]):
        raise _ffi.GdrError(f"kmeans_assign: centroids {tuple(centroids.shape)}, expected {(S * k, D.shape[1])}")
    if prev_labels is not None and (prev_labels.dtype != torch.int32 or prev_labels.numel() != n):
        raise _ffi.GdrError("kmeans_assign: prev_labels must be int32[n]")
    if work is None:
        work = kmeans_worklist(node_offsets, lib().gdr_kmeans_assign_tile())
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 2 or work.shape[0] == 0:
        raise _ffi.GdrError("kmeans_assign: work must be int32[n_work, 2]")
    dev = D.device
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    score = torch.empty((n,), dtype=torch.float32, device=dev)
    changed = torch.empty((S,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    need = lib().gdr_kmeans_assign_workspace_bytes(S, k)
    ws = (workspace or Workspace(dev)).get(need)
    check(lib().gdr_kmeans_assign(ptr(D), D.shape[0], D.shape[1], ptr(rows), n, ptr(node_offsets), S, ptr(centroids), k,
                                  ptr(work.contiguous()), work.shape[0], ptr(prev_labels.contiguous()) if prev_labels is not None else None,
                                  ptr(labels), ptr(score), ptr(changed), ptr(status), ptr(ws), ws.numel(), stream_ptr()),
          "gdr_kmeans_assign")
    return labels, score, changed, status


def kmeans_partition(rows, labels, node_offsets, k, work=None, workspace=None):
    """gdr_kmeans_partition: stable segmented counting sort of every node's rows by label -> (rows' int32[n], child_offsets
    int32[S*k+1], status int32[1]: bit 1 a label outside [0, k), bit 2 a malformed work item).  Child j of node s is
    rows'[child_offsets[s*k+j] : child_offsets[s*k+j+1]], ascending.  No read-back (beyond building the work list when absent)."""
    _kmeans_check("kmeans_partition", None, rows, node_offsets, k)
    _need_cuda(labels, work)
    n, S = rows.numel(), node_offsets.numel() - 1
    if labels.dtype != torch.int32 or labels.numel() != n:
        raise _ffi.GdrError("kmeans_partition: labels must be int32[n]")
    rows, labels, node_offsets = rows.contiguous(), labels.contiguous(), node_offsets.contiguous()
    if work is None:
        work = kmeans_worklist(node_offsets, lib().gdr_kmeans_partition_tile())
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 2 or work.shape[0] == 0:
        raise _ffi.GdrError("kmeans_partition: work must be int32[n_work, 2]")
    dev = rows.device
    out_rows = torch.empty((n,), dtype=torch.int32, device=dev)
    child = torch.empty((S * k + 1,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    need = lib().gdr_kmeans_partition_workspace_bytes(work.shape[0], k)
    ws = (workspace or Workspace(dev)).get(need)
    check(lib().gdr_kmeans_partition(ptr(rows), ptr(labels), n, ptr(node_offsets), S, k, ptr(work.contiguous()), work.shape[0],
                                     ptr(out_rows), ptr(child), ptr(status), ptr(ws), ws.numel(), stream_ptr()),
          "gdr_kmeans_partition")
    return out_rows, child, status


def kmeans_centroids(D, child_offsets, rows, workspace=None):
    """gdr_kmeans_centroids: the k-means update step over the child CSR of kmeans_partition -> (centroids fp32[C,d], counts
    int32[C]); member means as a fixed-shape two-stage sum (chunks of 256 members in order, then the chunk sums in order, one
    division): deterministic, and gdr_cluster_centroids' bits for a child of <= 256 members.  An empty child: count 0, zero row."""
    _need_cuda(D, child_offsets, rows)
    if D.dtype != torch.float32:
        raise _ffi.GdrError(f"kmeans_centroids: the corpus must be float32, got {D.dtype} (a bf16 corpus is not supported)")
    D = _f32c(D)
    if child_offsets.dtype != torch.int32 or rows.dtype != torch.int32:
        raise _ffi.GdrError("kmeans_centroids: expected int32 child_offsets / rows")
    N, d = D.shape
    C_, n = child_offsets.numel() - 1, rows.numel()
    if C_ < 1 or n < 1:
        raise _ffi.GdrError("kmeans_centroids: empty level")
    cent = torch.empty((C_, d), dtype=torch.float32, device=D.device)
    counts = torch.empty((C_,), dtype=torch.int32, device=D.device)
    need = lib().gdr_kmeans_centroids_workspace_bytes(n, d)
    ws = (workspace or Workspace(D.device)).get(need)
    check(lib().gdr_kmeans_centroids(ptr(D), N, d, ptr(child_offsets.contiguous()), ptr(rows.contiguous()), n, C_, ptr(cent),
                                     ptr(counts), ptr(ws), ws.numel(), stream_ptr()), "gdr_kmeans_centroids")
    return cent, counts


KMEANS_SEED_MAX_T = 6


def kmeans_seed_dist(D, rows, node_offsets, cand, d2, e, work=None, workspace=None):
    """gdr_kmeans_seed_dist: one greedy k-means++ step over the nodes of a level (include/gdr_hip_kmeans_seed.h).  cand int32[S, T]
    candidate doc ids (negative: none), d2 fp32[n] distance to the nearest chosen centre (+inf before the first), e int32[S] the
    nodes' exponents; work = kmeans_worklist(node_offsets, gdr_kmeans_seed_tile()) (built here when absent) -> (cand_d2 fp32[n, T] =
    min(d2, distance to the candidate), pot int64[n_work, T] and max fp32[n_work, T] per tile, status int32[1]).  No read-back."""
    _need_cuda(D, rows, node_offsets, cand, d2, e, work)
    if D.dtype != torch.float32:
        raise _ffi.GdrError(f"kmeans_seed_dist: the corpus must be float32, got {D.dtype} (a bf16 corpus is not supported)")
    if D.dim() != 2 or D.shape[1] % 4 or not 4 <= D.shape[1] <= KMEANS_MAX_D:
        raise _ffi.GdrError(f"kmeans_seed_dist: d={D.shape[-1]} (needs d % 4 == 0, 4 <= d <= {KMEANS_MAX_D})")
    if D.shape[0] >= 1 << 31:
        raise _ffi.GdrError(f"kmeans_seed_dist: N={D.shape[0]} does not fit int32 doc ids")
    for t in (rows, node_offsets, cand, e):
        if t.dtype != torch.int32:
            raise _ffi.GdrError(f"kmeans_seed_dist: expected int32, got {t.dtype}")
    if rows.numel() == 0 or node_offsets.numel() < 2:
        raise _ffi.GdrError("kmeans_seed_dist: empty level")
    D = _f32c(D)
    n, S = rows.numel(), node_offsets.numel() - 1
    if cand.dim() != 2 or cand.shape[0] != S or not 1 <= cand.shape[1] <= KMEANS_SEED_MAX_T:
        raise _ffi.GdrError(f"kmeans_seed_dist: cand {tuple(cand.shape)}, expected ({S}, 1..{KMEANS_SEED_MAX_T})")
    if d2.dtype != torch.float32 or d2.numel() != n or e.numel() != S:
        raise _ffi.GdrError("kmeans_seed_dist: d2 must be float32[n] and e int32[n_nodes]")
    T = cand.shape[1]
    if work is None:
        work = kmeans_worklist(node_offsets, lib().gdr_kmeans_seed_tile())
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 2 or work.shape[0] == 0:
        raise _ffi.GdrError("kmeans_seed_dist: work must be int32[n_work, 2]")
    dev = D.device
    W = work.shape[0]
    cand_d2 = torch.empty((n, T), dtype=torch.float32, device=dev)
    pot = torch.empty((W, T), dtype=torch.int64, device=dev)
    mx = torch.empty((W, T), dtype=torch.float32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    need = lib().gdr_kmeans_seed_workspace_bytes(S, W, T)
    ws = (workspace or Workspace(dev)).get(need) if need else None
    check(lib().gdr_kmeans_seed_dist(ptr(D), D.shape[0], D.shape[1], ptr(rows.contiguous()), n, ptr(node_offsets.contiguous()), S,
                                     ptr(work.contiguous()), W, ptr(cand.contiguous()), T, ptr(d2.contiguous()), ptr(e.contiguous()),
                                     ptr(cand_d2), ptr(pot), ptr(mx), ptr(status), ptr(ws), ws.numel() if ws is not None else 0,
                                     stream_ptr()), "gdr_kmeans_seed_dist")
    return cand_d2, pot, mx, status


def relative_bucket_table(bidirectional, num_buckets, max_distance, qlen, klen):
    """Host table int32[qlen,klen] from the same routine the attention kernels use (no GPU needed)."""
    buf = (C.c_int32 * (qlen * klen))()
    check(lib().gdr_t5_relative_bucket_table(int(bidirectional), num_buckets, max_distance, qlen, klen, buf),
          "gdr_t5_relative_bucket_table")
    return torch.tensor(list(buf), dtype=torch.int32).view(qlen, klen)


class T5EncoderHandle:
    """Device-resident encoder weights + the pointer table gdr_t5_encoder_forward reads.
    Built once from a reference-style state_dict; q/k/v are row-concatenated.
    dtype=torch.bfloat16 selects the C5 precision mode: the linear weights are rounded to bf16 on the device
    (gdr_cast_f32_bf16) and forward() calls gdr_t5_encoder_forward_bf16; everything else stays fp32."""

    def __init__(self, cfg, sd, device, prefix="encoder.", dtype=torch.float32, split=False, token_table=None):
        """token_table (float32 without split, d_kv = 64): block 0's q/k/v of every token id, [vocab, 3*inner] fp32 made once here
        (T5 adds no position embedding, so they depend on the id alone); the ragged forward gathers them instead of running block 0's
        norm and qkv linear (include/gdr_hip.h).  Default on; token_table=False or GDR_ENC_TOKEN_TABLE=0 leaves it out (the exact
        A/B switch).  It is a snapshot of the weights: after an in-place update call refresh_token_table().
        split=True (r06, exploratory; dtype float32): every linear weight is stored as three bf16 planes (split_bf16x3) and forward()
        runs gdr_t5_encoder_forward_ragged_split — fp32 operands carried through bf16 MFMAs with fp32-level error, not fp32 bits.
        split=2 (fp16 x 2 planes): an operand |x| in [2^-14, 65504] is carried to 2^-21 relative, a smaller one to an absolute 3e-11,
        and one >= 65520 overflows fp16 and makes its output row non-finite (never a finite wrong value)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("T5EncoderHandle: dtype must be float32 or bfloat16")
        if split and dtype != torch.float32:
            raise ValueError("T5EncoderHandle: split=True is a form of the float32 mode")
        if split not in (False, True, 0, 2, 3, 6):
            raise ValueError("T5EncoderHandle: split must be False, True (= 6 terms), 3 / 6 (bf16 planes) or 2 (fp16 x 2)")
        self.cfg, self.device, self.dtype, self.split = cfg, device, dtype, (6 if split is True else int(split))
        keep = []

        def dev(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t

        def lin(t):                                      # a linear's weight: bf16 copy in the C5 mode, three bf16 planes in the split form
            t = dev(t)
            if dtype == torch.bfloat16:
                keep.pop()
                t = to_bf16(t)
                keep.append(t)
            elif split:
                keep.pop()
                t = split_f16x2(t) if int(split) == 2 else split_bf16x3(t)
                keep.append(t)
            return t

        self.embed = dev(sd["shared.weight"] if "shared.weight" in sd else sd[prefix + "embed_tokens.weight"])
        self.rel_bias = dev(sd[prefix + "block.0.layer.0.SelfAttention.relative_attention_bias.weight"])
        self.final_ln = dev(sd[prefix + "final_layer_norm.weight"])
        nl = cfg.num_layers
        self._layers = (_ffi.GdrT5EncLayer * nl)()
        for i in range(nl):
            p = f"{prefix}block.{i}.layer."
            wqkv = lin(torch.cat([sd[p + "0.SelfAttention.q.weight"], sd[p + "0.SelfAttention.k.weight"],
                                  sd[p + "0.SelfAttention.v.weight"]], dim=0))
            L = self._layers[i]
            ln_attn = dev(sd[p + "0.layer_norm.weight"])
            if i == 0:
                self._ln0, self._wqkv0 = ln_attn, wqkv       # what the token table is made from
            L.ln_attn = ln_attn.data_ptr()
            L.wqkv = wqkv.data_ptr()
            L.wo = lin(sd[p + "0.SelfAttention.o.weight"]).data_ptr()
            L.ln_ff = dev(sd[p + "1.layer_norm.weight"]).data_ptr()
            L.wi = lin(sd[p + "1.DenseReluDense.wi.weight"]).data_ptr()
            L.wo_ff = lin(sd[p + "1.DenseReluDense.wo.weight"]).data_ptr()
        self._keep = keep
        self.dims = _ffi.GdrT5Dims(cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_heads, nl,
                                   cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance,
                                   cfg.layer_norm_epsilon)
        self.struct = _ffi.GdrT5EncoderWeights(self.dims, self.embed.data_ptr(), self.rel_bias.data_ptr(),
                                               self.final_ln.data_ptr(), self._layers)
        self.ws = Workspace(device)
        if token_table is None:
            token_table = os.environ.get("GDR_ENC_TOKEN_TABLE", "1") != "0"
        inner = cfg.num_heads * cfg.d_kv
        # only the packed un-split form reads the table (csrc/encoder.hip ragged_packs): other precisions and widths never would
        packs = cfg.d_kv == 64 and cfg.d_model % 32 == 0 and cfg.d_ff % 32 == 0 and inner % 32 == 0
        self.token_table = None
        if token_table and dtype == torch.float32 and not split and packs:
            self.token_table = torch.empty((cfg.vocab_size, 3 * inner), dtype=torch.float32, device=device)
            self.refresh_token_table()
            self.struct.qkv0_table = self.token_table.data_ptr()

    @property
    def token_table_bytes(self):
        """Device memory the token table adds (0 without one): vocab * 3 * inner * 4."""
        return 0 if self.token_table is None else self.token_table.numel() * 4

    def refresh_token_table(self, chunk=4096):
        """Re-derive the token table from the current embedding, block 0's norm weight and wqkv (after an in-place weight update,
        like PrefilteredCorpus.refresh()).  table[id] = t5_layer_norm(embed[id]) @ wqkv0.T with the operators the encoder itself
        launches, so a row holds the bits the in-encoder launch gives; built in row chunks (temporary: chunk * d_model floats)."""
        if self.token_table is None:
            return self
        for s in range(0, self.cfg.vocab_size, chunk):
            e = min(s + chunk, self.cfg.vocab_size)
            linear(t5_layer_norm(self.embed[s:e], self._ln0, self.cfg.layer_norm_epsilon), self._wqkv0, out=self.token_table[s:e])
        return self

    def forward(self, input_ids, attention_mask=None, want_pooled=True, want_hidden=True, ragged=False,
                live_rows_hint=-1):
        """Returns (last_hidden_state fp32[B,L,d] | None, pooled fp32[B,d] | None).
        ragged=False: gdr_t5_encoder_forward — every row, PAD positions included, exactly as the reference computes them.
        ragged=True : gdr_t5_encoder_forward_ragged — PAD rows are not computed (kept rows bit-identical, PAD rows of the
        returned hidden states are zero); with want_hidden=False only h[:,0] is carried through the last block.
        live_rows_hint: number of kept token rows if the caller knows it — a tuning input (the launcher chooses between
        bit-identical kernel forms by the tile count it implies; the profiler prices flops with it), never a result input."""
        _need_cuda(input_ids, attention_mask)
        ids = input_ids.to(torch.int64).contiguous()
        B, L = ids.shape
        if attention_mask is None:
            attention_mask = torch.ones_like(ids)
        mask = attention_mask.to(torch.int64).contiguous()
        bf = self.dtype == torch.bfloat16
        if not (want_hidden or want_pooled):
            raise ValueError("T5EncoderHandle.forward: nothing requested")
        d = self.cfg.d_model
        pooled = torch.empty((B, d), dtype=torch.float32, device=ids.device) if want_pooled else None
        if self.split:
            if not ragged:
                raise _ffi.GdrError("T5EncoderHandle(split=True): the split form exists for the ragged forward only")
            need = lib().gdr_t5_encoder_split_workspace_bytes(C.byref(self.dims), B, L)
            ws = self.ws.get(need)
            out = torch.empty((B, L, d), dtype=torch.float32, device=ids.device) if want_hidden else None
            check(lib().gdr_t5_encoder_forward_ragged_split(C.byref(self.struct), ptr(ids), ptr(mask), B, L, ptr(out), ptr(pooled),
                                                            int(live_rows_hint), self.split, ptr(ws), ws.numel(), stream_ptr()),
                  "gdr_t5_encoder_forward_ragged_split")
            return out, pooled
        if ragged:
            need = lib().gdr_t5_encoder_ragged_workspace_bytes(C.byref(self.dims), B, L)
            ws = self.ws.get(need)
            out = torch.empty((B, L, d), dtype=torch.float32, device=ids.device) if want_hidden else None
            rfn = lib().gdr_t5_encoder_forward_ragged_bf16 if bf else lib().gdr_t5_encoder_forward_ragged
            check(rfn(C.byref(self.struct), ptr(ids), ptr(mask), B, L, ptr(out), ptr(pooled), int(live_rows_hint), ptr(ws),
                      ws.numel(), stream_ptr()), "gdr_t5_encoder_forward_ragged")
            return out, pooled
        need = (lib().gdr_t5_encoder_bf16_workspace_bytes if bf else lib().gdr_t5_encoder_workspace_bytes)(
            C.byref(self.dims), B, L)
        ws = self.ws.get(need)
        out = torch.empty((B, L, d), dtype=torch.float32, device=ids.device)
        fn = lib().gdr_t5_encoder_forward_bf16 if bf else lib().gdr_t5_encoder_forward
        check(fn(C.byref(self.struct), ptr(ids), ptr(mask), B, L, ptr(out), ptr(pooled), ptr(ws), ws.numel(),
                 stream_ptr()), "gdr_t5_encoder_forward")
        return (out if want_hidden else None), pooled


BERT_MAX_LEN = 512             # the doc tower's entry points take L <= min(BERT_MAX_LEN, max_pos) (csrc/bert.hip)
T5_MAX_LEN = 512               # input tokens per sequence in every T5 encoder form and in generate() (csrc/attention.h T5_MAX_LEN)
ATTN_LONG_QUERY_BLOCK = 128    # above 128 tokens (csrc/attention_long.hip): query rows per workgroup ...
ATTN_LONG_KEY_BLOCK = 64       # ... and keys per staged K / V block; stated here for the tests that walk the block edges


class BertEncoderHandle:
    """Device-resident doc-tower weights (DPRContextEncoder / BertModel keys) + pointer table.
    Passages of up to BERT_MAX_LEN = 512 tokens (the reference's corpus embedder runs at MAX_LEN=512), bounded by max_pos.
    dtype=torch.bfloat16 selects the bf16 precision mode (config C5's corpus is bf16): the linear weights are rounded to bf16 on the
    device, the attention's 1/sqrt(dh) is folded into the q rows of wqkv / bqkv (exact: a power of two at dh = 64), and forward()
    runs gdr_bert_encoder_forward_ragged_bf16 — the packed form is the only bf16 form."""

    def __init__(self, bcfg, sd, device, prefix="ctx_encoder.bert_model.", dtype=torch.float32, split=False):
        """split=True (r06, exploratory; dtype float32): the linear weights are stored as fp16 x 2 plane rows (split_f16x2) and forward()
        runs gdr_bert_encoder_forward_ragged_split — fp32-level embeddings through the fp16 MFMA path.  An operand |x| in
        [2^-14, 65504] is carried to 2^-21 relative, a smaller one to an absolute 3e-11, and one >= 65520 overflows fp16 and makes its
        output row non-finite (never a finite wrong value)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("BertEncoderHandle: dtype must be float32 or bfloat16")
        if split and dtype != torch.float32:
            raise ValueError("BertEncoderHandle: split=True is a form of the float32 mode")
        self.bcfg, self.device, self.dtype, self.split = bcfg, device, dtype, bool(split)
        bf = dtype == torch.bfloat16
        keep = []

        def dev(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t

        def lin(t):                                      # a linear's weight: bf16 copy in the bf16 mode
            t = dev(t)
            if bf:
                keep.pop()
                t = to_bf16(t)
                keep.append(t)
            elif split:
                keep.pop()
                t = split_f16x2(t)
                keep.append(t)
            return t

        d, H = bcfg["hidden_size"], bcfg["num_heads"]
        qs = 1.0
        if bf:
            dh = d // H
            qs = float(dh) ** -0.5
            if d % H or 2.0 ** round(math.log2(qs)) != qs:
                raise _ffi.GdrError(f"BertEncoderHandle(bf16): head width {dh} — the scale fold needs 1/sqrt(dh) to be a power of two")
        e = prefix + "embeddings."
        self.word, self.pos = dev(sd[e + "word_embeddings.weight"]), dev(sd[e + "position_embeddings.weight"])
        self.type = dev(sd[e + "token_type_embeddings.weight"])
        self.eln_w, self.eln_b = dev(sd[e + "LayerNorm.weight"]), dev(sd[e + "LayerNorm.bias"])
        nl = bcfg["num_layers"]
        self._layers = (_ffi.GdrBertLayer * nl)()
        for i in range(nl):
            p = f"{prefix}encoder.layer.{i}."
            L = self._layers[i]
            wq, bq = sd[p + "attention.self.query.weight"] * qs, sd[p + "attention.self.query.bias"] * qs
            L.wqkv = lin(torch.cat([wq] + [sd[p + f"attention.self.{n}.weight"] for n in ("key", "value")], 0)).data_ptr()
            L.bqkv = dev(torch.cat([bq] + [sd[p + f"attention.self.{n}.bias"] for n in ("key", "value")], 0)).data_ptr()
            L.wo, L.bo = lin(sd[p + "attention.output.dense.weight"]).data_ptr(), dev(sd[p + "attention.output.dense.bias"]).data_ptr()
            L.ln1_w = dev(sd[p + "attention.output.LayerNorm.weight"]).data_ptr()
            L.ln1_b = dev(sd[p + "attention.output.LayerNorm.bias"]).data_ptr()
            L.wi, L.bi = lin(sd[p + "intermediate.dense.weight"]).data_ptr(), dev(sd[p + "intermediate.dense.bias"]).data_ptr()
            L.wo2, L.bo2 = lin(sd[p + "output.dense.weight"]).data_ptr(), dev(sd[p + "output.dense.bias"]).data_ptr()
            L.ln2_w, L.ln2_b = dev(sd[p + "output.LayerNorm.weight"]).data_ptr(), dev(sd[p + "output.LayerNorm.bias"]).data_ptr()
        self._keep = keep
        self.struct = _ffi.GdrBertWeights(self.word.shape[0], bcfg["hidden_size"], bcfg["num_heads"], bcfg["d_ff"], nl,
                                          self.pos.shape[0], self.type.shape[0], bcfg["eps"], self.word.data_ptr(),
                                          self.pos.data_ptr(), self.type.data_ptr(), self.eln_w.data_ptr(),
                                          self.eln_b.data_ptr(), self._layers)
        self.ws = Workspace(device)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, want_hidden=True, ragged=None, live_rows_hint=-1):
        """Returns (sequence_output fp32[B,L,d] | None, pooled fp32[B,d]).
        ragged=False: gdr_bert_encoder_forward — every position of every passage, as the reference computes them.
        ragged=True : gdr_bert_encoder_forward_ragged — PAD rows are not computed (kept rows bit-identical, PAD rows of the returned
        hidden states zero); with want_hidden=False only the CLS rows go through the last block.  Default: ragged for the bf16
        mode (its only form), padded otherwise."""
        _need_cuda(input_ids, attention_mask, token_type_ids)
        bf = self.dtype == torch.bfloat16
        ragged = (bf or self.split) if ragged is None else ragged
        if (bf or self.split) and not ragged:
            raise _ffi.GdrError("BertEncoderHandle: the bf16 precision mode and the split form exist in the packed (ragged) form only")
        ids = input_ids.to(torch.int64).contiguous()
        B, L = ids.shape
        mask = (torch.ones_like(ids) if attention_mask is None else attention_mask.to(torch.int64)).contiguous()
        tt = None if token_type_ids is None else token_type_ids.to(torch.int64).contiguous()
        d = self.bcfg["hidden_size"]
        hid = torch.empty((B, L, d), dtype=torch.float32, device=ids.device) if want_hidden else None
        pooled = torch.empty((B, d), dtype=torch.float32, device=ids.device)
        if ragged:
            need = lib().gdr_bert_encoder_ragged_workspace_bytes(C.byref(self.struct), B, L)
            ws = self.ws.get(need)
            fn = (lib().gdr_bert_encoder_forward_ragged_bf16 if bf else lib().gdr_bert_encoder_forward_ragged_split if self.split
                  else lib().gdr_bert_encoder_forward_ragged)
            check(fn(C.byref(self.struct), ptr(ids), ptr(mask), ptr(tt), B, L, ptr(hid), ptr(pooled), int(live_rows_hint), ptr(ws),
                     ws.numel(), stream_ptr()), "gdr_bert_encoder_forward_ragged")
            return hid, pooled
        need = lib().gdr_bert_encoder_workspace_bytes(C.byref(self.struct), B, L)
        ws = self.ws.get(need)
        check(lib().gdr_bert_encoder_forward(C.byref(self.struct), ptr(ids), ptr(mask), ptr(tt), B, L, ptr(hid), ptr(pooled),
                                             ptr(ws), ws.numel(), stream_ptr()), "gdr_bert_encoder_forward")
        return hid, pooled


class T5DecoderHandle:
    """Device-resident decoder + adaptor + head weights and the pointer table gdr_t5_generate reads.
    Load-time re-layouts (pure data movement / weight-only algebra, done once):
      * q,k,v of self-attention row-concatenated; k,v of cross-attention row-concatenated;
      * adaptor_linear.weight [d*Vd, d] (= [i, c, k], modeling_t5.py:1634-1636) sliced per decode position into
        head_w[p][c'][i][k] for the V+1 columns that survive the positional mask (modeling_t5.py:1553-1557);
      * the adaptor's cross-attention over its single learned key folded into cross_const (softmax of one key = 1).
    An adaptor-free config (cfg.has_adaptor False: --adaptor_decode 0 --adaptor_efficient 0) builds the plain form of
    GdrT5DecoderWeights: no adaptor* key is read, head_w is None and only head_e (lm_head's rows per position) is resident.
    The state dict must match the config either way — adaptor weights under an adaptor-free config, or none under an adaptor
    config, raise GdrError naming the key: a different model is never run silently."""

    def __init__(self, cfg, sd, device, dtype=torch.float32):
        """dtype=torch.bfloat16: the C5 precision mode — every linear weight (decoder, adaptor, head slices) is rounded to
        bf16 on the device and generate() calls gdr_t5_generate_bf16; everything else stays fp32."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("T5DecoderHandle: dtype must be float32 or bfloat16")
        self.cfg, self.device, self.dtype = cfg, device, dtype
        keep = []

        def dev(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t

        def lin(t):                                      # a linear's weight: bf16 copy in the C5 mode
            t = dev(t)
            if dtype == torch.bfloat16:
                keep.pop()
                t = to_bf16(t)
                keep.append(t)
            return t

        d, V, Vd, ml = cfg.d_model, cfg.output_vocab_size, cfg.decode_vocab_size, cfg.max_output_length
        nl, na = cfg.num_decoder_layers, (cfg.adaptor_layer_num if cfg.has_adaptor else 0)
        if cfg.has_adaptor:
            need = ["adaptor_embeddings", "adaptor_linear.weight"] + [f"adaptor.layers.{i}.self_attn.in_proj_weight" for i in range(na)]
            for k in need:
                if k not in sd:
                    raise _ffi.GdrError(f"T5DecoderHandle: the state dict has no {k!r} but the config has the adaptor head "
                                        "(adaptor_decode=1, adaptor_efficient=1); an adaptor-free checkpoint needs "
                                        "GDRConfig(adaptor_decode=0, adaptor_efficient=0)")
        else:
            for k in sd:
                if k.startswith(("adaptor_linear.", "adaptor.layers.", "adaptor_embeddings")):
                    raise _ffi.GdrError(f"T5DecoderHandle: the state dict holds {k!r} but the config is adaptor-free "
                                        "(adaptor_decode=0, adaptor_efficient=0): refusing to drop trained adaptor weights")
        self.dec_embed = dev(sd["decode_embeddings.weight"])
        self.self_rel = dev(sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"])
        self.cross_rel = dev(sd["decoder.block.0.layer.1.EncDecAttention.relative_attention_bias.weight"])
        self.final_ln = dev(sd["decoder.final_layer_norm.weight"])
        self._layers = (_ffi.GdrT5DecLayer * nl)()
        for i in range(nl):
            p = f"decoder.block.{i}.layer."
            L = self._layers[i]
            L.ln_self = dev(sd[p + "0.layer_norm.weight"]).data_ptr()
            L.wqkv = lin(torch.cat([sd[p + "0.SelfAttention.q.weight"], sd[p + "0.SelfAttention.k.weight"],
                                    sd[p + "0.SelfAttention.v.weight"]], dim=0)).data_ptr()
            L.wo = lin(sd[p + "0.SelfAttention.o.weight"]).data_ptr()
            L.ln_cross = dev(sd[p + "1.layer_norm.weight"]).data_ptr()
            L.wq_c = lin(sd[p + "1.EncDecAttention.q.weight"]).data_ptr()
            L.wkv_c = lin(torch.cat([sd[p + "1.EncDecAttention.k.weight"], sd[p + "1.EncDecAttention.v.weight"]],
                                    dim=0)).data_ptr()
            L.wo_c = lin(sd[p + "1.EncDecAttention.o.weight"]).data_ptr()
            L.ln_ff = dev(sd[p + "2.layer_norm.weight"]).data_ptr()
            L.wi = lin(sd[p + "2.DenseReluDense.wi.weight"]).data_ptr()
            L.wo_ff = lin(sd[p + "2.DenseReluDense.wo.weight"]).data_ptr()
        mem = dev(sd["adaptor_embeddings"]).view(1, d) if na else None
        self._alayers = (_ffi.GdrAdaptorLayer * na)() if na else None
        aff = None
        for i in range(na):
            p = f"adaptor.layers.{i}."
            A = self._alayers[i]
            A.in_w = lin(sd[p + "self_attn.in_proj_weight"]).data_ptr()
            A.in_b = dev(sd[p + "self_attn.in_proj_bias"]).data_ptr()
            A.out_w = lin(sd[p + "self_attn.out_proj.weight"]).data_ptr()
            A.out_b = dev(sd[p + "self_attn.out_proj.bias"]).data_ptr()
            cw, cb = dev(sd[p + "multihead_attn.in_proj_weight"]), dev(sd[p + "multihead_attn.in_proj_bias"])
            flin = linear_bf16 if dtype == torch.bfloat16 else linear        # the two folded linears round like all others
            vmem = flin(mem, cw[2 * d:].contiguous(), epilogue=_ffi.EPI_BIAS, bias=cb[2 * d:].contiguous())
            cc = flin(vmem, dev(sd[p + "multihead_attn.out_proj.weight"]), epilogue=_ffi.EPI_BIAS,
                      bias=dev(sd[p + "multihead_attn.out_proj.bias"]))
            keep.append(cc)
            A.cross_const = cc.data_ptr()
            for n in ("1", "2", "3"):
                setattr(A, f"ln{n}_w", dev(sd[p + f"norm{n}.weight"]).data_ptr())
                setattr(A, f"ln{n}_b", dev(sd[p + f"norm{n}.bias"]).data_ptr())
            l1 = lin(sd[p + "linear1.weight"])
            aff = l1.shape[0]
            A.lin1_w, A.lin1_b = l1.data_ptr(), dev(sd[p + "linear1.bias"]).data_ptr()
            A.lin2_w, A.lin2_b = lin(sd[p + "linear2.weight"]).data_ptr(), dev(sd[p + "linear2.bias"]).data_ptr()
        # head slices
        P = ml - 1
        cols = torch.tensor([[p * V + 2 + c for c in range(V)] + [1] for p in range(P)], dtype=torch.long, device=device)
        self.head_w = None                                   # adaptor-free: the head is head_e alone (head_plain_kernel)
        if na:
            Wfull = sd["adaptor_linear.weight"].detach().to(device=device, dtype=torch.float32)
            W = Wfull.view(d, Vd, d)
            self.head_w = torch.empty((P, V + 1, d, d), dtype=dtype, device=device)
            for p in range(P):                                   # per position: bounded temporaries
                sl = W[:, cols[p], :].permute(1, 0, 2).contiguous()
                self.head_w[p] = to_bf16(sl) if dtype == torch.bfloat16 else sl
            del W, Wfull                                         # only the slices stay resident
        self.head_e = dev(sd["lm_head.weight"])[cols].contiguous()            # [P, V+1, d]
        self._keep = keep
        self.dims = _ffi.GdrT5Dims(Vd, d, cfg.d_kv, cfg.d_ff, cfg.num_heads, nl, cfg.relative_attention_num_buckets,
                                   cfg.relative_attention_max_distance, cfg.layer_norm_epsilon)
        self.struct = _ffi.GdrT5DecoderWeights(self.dims, V, ml, na, cfg.adaptor_nhead if na else 0, aff or 0,
                                               cfg.adaptor_ln_eps if na else 0.0,
                                               self.dec_embed.data_ptr(), self.self_rel.data_ptr(),
                                               self.cross_rel.data_ptr(), self.final_ln.data_ptr(), self._layers,
                                               self._alayers, self.head_w.data_ptr() if na else None, self.head_e.data_ptr())
        self.ws = Workspace(device)

    def generate(self, enc_hidden, enc_mask, num_beams, max_length, length_penalty, num_return_sequences, trace=False,
                 trie=None, prefix_table=None, graph=False):
        """Returns (out_ids int64[B*nret,max_length], out_len int32[B*nret], out_scores float64[B*nret][, trace]).
        num_beams=1: greedy decode (include/gdr_hip.h) — nret must be 1, no trie and no trace; out_len counts START and EOS
        (max_length for a row without EOS) and out_scores is 0.
        graph=True: the ~1 400 kernel launches of one call are captured once per (B, L, beams, max_length, nret) into a HIP
        graph (gdr_t5_generate contains no host synchronisation and forks / joins its side stream with events, i.e. it is
        capturable as is) and replayed on later calls — at small batches (one query x 100 beams, infer.sh's setting) the
        call is otherwise bound by the host's launch rate, not by the GPU."""
        _need_cuda(enc_hidden, enc_mask)
        if prefix_table is not None and self.head_w is None:
            raise _ffi.GdrError("generate: a prefix table cannot be used with an adaptor-free model (it stores adaptor results)")
        enc_hidden = _f32c(enc_hidden)
        mask = enc_mask.to(torch.int64).contiguous()
        B, L, _ = enc_hidden.shape
        R, nret = int(num_beams), int(num_return_sequences)
        dev_ = enc_hidden.device
        fn = lib().gdr_t5_generate_bf16 if self.dtype == torch.bfloat16 else lib().gdr_t5_generate
        need = lib().gdr_t5_generate_workspace_bytes(C.byref(self.struct), B, L, R, max_length)

        def call(enc_t, mask_t, ids, lens, scores, ts, tt, ws):
            check(fn(C.byref(self.struct), ptr(enc_t), ptr(mask_t), B, L, R, max_length,
                     float(length_penalty), nret, trie.struct_ref() if trie is not None else None,
                     prefix_table.struct_ref() if prefix_table is not None else None,
                     ptr(ids), ptr(lens), ptr(scores), ptr(ts), ptr(tt),
                     ptr(ws), ws.numel(), stream_ptr()), "gdr_t5_generate")

        def outputs():
            ids = torch.empty((B * nret, max_length), dtype=torch.int64, device=dev_)
            lens = torch.empty((B * nret,), dtype=torch.int32, device=dev_)
            scores = torch.empty((B * nret,), dtype=torch.float64, device=dev_)
            return ids, lens, scores

        if graph and not trace:
            # one graph (and one set of static buffers) per call shape AND per stream: calls in flight on different
            # streams (GDRRetriever.validation_steps) replay different instances
            key = (B, L, R, max_length, nret, float(length_penalty), id(trie), id(prefix_table),
                   torch.cuda.current_stream(dev_).cuda_stream)
            if not hasattr(self, "_graphs"):
                self._graphs = {}
            entry = self._graphs.get(key)
            if entry is None:
                s_enc, s_mask = torch.empty_like(enc_hidden), torch.empty_like(mask)
                s_ids, s_lens, s_scores = outputs()
                s_ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev_)
                s_enc.copy_(enc_hidden)
                s_mask.copy_(mask)
                warm = torch.cuda.Stream(device=dev_)                 # capture needs one eager run first (kernel
                warm.wait_stream(torch.cuda.current_stream())         # attributes, the side-stream lease, lazy module loads)
                with torch.cuda.stream(warm):
                    call(s_enc, s_mask, s_ids, s_lens, s_scores, None, None, s_ws)
                torch.cuda.current_stream().wait_stream(warm)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    call(s_enc, s_mask, s_ids, s_lens, s_scores, None, None, s_ws)
                entry = self._graphs[key] = (g, s_enc, s_mask, s_ids, s_lens, s_scores, s_ws)
            g, s_enc, s_mask, s_ids, s_lens, s_scores, _ = entry
            s_enc.copy_(enc_hidden)
            s_mask.copy_(mask)
            g.replay()
            return s_ids.clone(), s_lens.clone(), s_scores.clone()

        ws = self.ws.get(need)
        ids, lens, scores = outputs()
        ts = tt = None
        if trace:
            ts = torch.empty((max_length - 1, B, 2 * R), dtype=torch.float32, device=dev_)
            tt = torch.empty((max_length - 1, B, 2 * R), dtype=torch.int32, device=dev_)
        call(enc_hidden, mask, ids, lens, scores, ts, tt, ws)
        return (ids, lens, scores, ts, tt) if trace else (ids, lens, scores)

    def score(self, enc_hidden, enc_mask, ids, rows_per_query, length_penalty, hidden=False):
        """Teacher forcing — gdr_t5_generate's score mode (out_len = NULL, include/gdr_hip.h): the decoder runs over the GIVEN docid
        rows `ids` int64[B*rows_per_query, max_length] (START, tokens, EOS, then PAD: what generate() returns at
        num_return_sequences == num_beams; row b*rows_per_query + r belongs to query b) and returns the score generate() reports for
        each of them, float64[rows].  hidden=True also returns the decoder's last hidden states: (scores, trace fp32[max_length,
        rows, d] — zero behind a row's first EOS —, the state at the first EOS fp32[rows, d] — zero without one —, the mean over the
        row's START and non-PAD positions fp32[rows, d]).  `ids` is only read.  No host synchronisation."""
        _need_cuda(enc_hidden, enc_mask, ids)
        if enc_hidden.dim() != 3 or enc_hidden.shape[2] != self.cfg.d_model:
            raise ValueError(f"score: enc_hidden must be [B, L, {self.cfg.d_model}], got {tuple(enc_hidden.shape)}")
        B, L, d = enc_hidden.shape
        R = int(rows_per_query)
        if tuple(enc_mask.shape) != (B, L):
            raise ValueError(f"score: enc_mask must be [{B}, {L}], got {tuple(enc_mask.shape)}")
        if ids.dtype != torch.int64:
            raise TypeError(f"score: ids must be int64 (generate()'s out_ids), got {ids.dtype}")
        if R < 1 or ids.dim() != 2 or ids.shape[0] != B * R:
            raise ValueError(f"score: ids must be [B*rows_per_query = {B * R}, max_length], got {tuple(ids.shape)}")
        max_length = int(ids.shape[1])
        enc_hidden = _f32c(enc_hidden)
        mask = enc_mask.to(torch.int64).contiguous()
        ids = ids.contiguous()
        dev_ = enc_hidden.device
        fn = lib().gdr_t5_generate_bf16 if self.dtype == torch.bfloat16 else lib().gdr_t5_generate
        ws = self.ws.get(lib().gdr_t5_generate_workspace_bytes(C.byref(self.struct), B, L, R, max_length))
        scores = torch.empty((B * R,), dtype=torch.float64, device=dev_)
        planes = torch.empty((max_length + 2, B * R, d), dtype=torch.float32, device=dev_) if hidden else None
        check(fn(C.byref(self.struct), ptr(enc_hidden), ptr(mask), B, L, R, max_length, float(length_penalty), R, None, None,
                 ptr(ids), None, ptr(scores), ptr(planes), None, ptr(ws), ws.numel(), stream_ptr()), "gdr_t5_generate")
        return (scores, planes[:max_length], planes[max_length], planes[max_length + 1]) if hidden else scores


class DeviceTrie:
    """codec.Trie arrays resident on the GPU + the GdrTrie struct."""

    def __init__(self, trie, device):
        self.child = torch.from_numpy(trie.child).to(device).contiguous()
        self.eos_ok = torch.from_numpy(trie.eos_ok).to(device).contiguous()
        self.struct = _ffi.GdrTrie(self.child.data_ptr(), self.eos_ok.data_ptr(), self.child.shape[0], int(trie.V))

    def struct_ref(self):
        return C.byref(self.struct)


class PrefixTable:
    """Device prefix table (include/gdr_hip.h GdrPrefixTable) over a docid trie, built once from the decoder handle's
    weights by gdr_t5_prefix_table_build: per trie node the adaptor's per-layer (q,k,v) and the head matrix
    W = adaptor_linear(adaptor(prefix)) + lm_head of the node's position (modeling_t5.py:1618-1639, query-independent).
    `trie` is a codec.Trie in any order; `.device_trie` is its breadth-first DeviceTrie — pass THAT one as the constraint
    trie when both are used (gdr_t5_generate checks that they share their arrays)."""

    def __init__(self, dec, trie, device, max_levels=None, max_bytes=None, kv=None, W=None, workspace=None):
        """max_levels: cap on the trie depth stored.  max_bytes: HBM budget of the table (default: half of what is free on
        the device now) — the table costs n_table * (adaptor_layers*3*d + (V+1)*d) * 4 bytes (~130 KB per node at t5-base),
        so the deepest levels are dropped until it fits (rows whose prefix is deeper simply take the computed path);
        a table that does not even hold the root level raises.
        kv, W (optional): caller-provided table storage, fp32 [adaptor_layers, n_table, 3d] and [n_table, V+1, d]; workspace
        (optional): an object whose get(nbytes) returns the build's scratch (ops.Workspace).  Defaults: allocated here."""
        import numpy as np
        cfg = dec.cfg
        if not cfg.has_adaptor:
            raise _ffi.GdrError("PrefixTable: the model has no adaptor (adaptor_decode=0, adaptor_efficient=0) — the table stores the "
                                "adaptor's query-independent results and the plain lm_head head has none")
        bfs, level_off, parent, tok = trie.breadth_first()
        n_levels = min(len(level_off) - 1, cfg.max_output_length - 1, max_levels or (1 << 30))
        per_node = (cfg.adaptor_layer_num * 3 * cfg.d_model + (cfg.output_vocab_size + 1) * cfg.d_model) * 4
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(device)[0] // 2
        full = n_levels
        while n_levels > 1 and int(level_off[n_levels]) * per_node > max_bytes:
            n_levels -= 1
        if int(level_off[n_levels]) * per_node > max_bytes:
            raise _ffi.GdrError(f"PrefixTable: even {int(level_off[n_levels])} nodes need more than the {max_bytes >> 20} MiB budget")
        if n_levels < full:
            print(f"[gdr_amd] prefix table: {int(level_off[full])} trie nodes would need "
                  f"{int(level_off[full]) * per_node / 2**30:.1f} GiB; keeping the first {n_levels} of {full} levels "
                  f"({int(level_off[n_levels])} nodes, {int(level_off[n_levels]) * per_node / 2**30:.2f} GiB) — deeper prefixes are computed")
        n_table = int(level_off[n_levels])
        self.device_trie = DeviceTrie(bfs, device)
        anc_blocks, anc = [], np.zeros((1, 1), np.int32)                 # level 0: the root's ancestor list is itself
        for s in range(n_levels):
            lo, hi = int(level_off[s]), int(level_off[s + 1])
            if s > 0:
                anc = np.concatenate([anc[parent[lo:hi] - int(level_off[s - 1])], np.arange(lo, hi, dtype=np.int32)[:, None]], 1)
            anc_blocks.append(anc.reshape(-1))
        node_anc = torch.from_numpy(np.concatenate(anc_blocks).astype(np.int32)).to(device)
        node_tok = torch.from_numpy(tok[:n_table].copy()).to(device)
        d, V1, na = cfg.d_model, cfg.output_vocab_size + 1, cfg.adaptor_layer_num
        for name, t, shape in (("kv", kv, (na, n_table, 3 * d)), ("W", W, (n_table, V1, d))):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
                raise _ffi.GdrError(f"PrefixTable: {name} must be a contiguous float32 tensor of shape {shape}")
        self.kv = kv if kv is not None else torch.empty((na, n_table, 3 * d), dtype=torch.float32, device=device)
        self.W = W if W is not None else torch.empty((n_table, V1, d), dtype=torch.float32, device=device)
        lo_host = (C.c_int32 * (n_levels + 1))(*[int(x) for x in level_off[:n_levels + 1]])
        max_n = int(max(level_off[s + 1] - level_off[s] for s in range(n_levels)))
        need = lib().gdr_t5_prefix_table_workspace_bytes(C.byref(dec.struct), max_n)
        ws = workspace.get(need) if workspace is not None else torch.empty(need, dtype=torch.uint8, device=device)
        build = lib().gdr_t5_prefix_table_build_bf16 if dec.dtype == torch.bfloat16 else lib().gdr_t5_prefix_table_build
        check(build(C.byref(dec.struct), n_levels, lo_host, ptr(node_tok), ptr(node_anc), ptr(self.kv), ptr(self.W), ptr(ws),
                    ws.numel(), stream_ptr()), "gdr_t5_prefix_table_build")
        torch.cuda.current_stream().synchronize()                        # the scratch tensors above may go now
        self.n_levels, self.n_table, self.level_off = n_levels, n_table, level_off
        # levels 0 .. c-1 hold ALL V^s prefixes of their length (and are inside the table): no beam row can miss at those steps
        c = 1
        while c < n_levels and int(level_off[c + 1]) - int(level_off[c]) == int(bfs.V) ** c:
            c += 1
        self.complete_levels = c
        self.struct = _ffi.GdrPrefixTable(self.device_trie.child.data_ptr(), self.device_trie.child.shape[0], int(bfs.V),
                                          n_table, self.kv.data_ptr(), self.W.data_ptr(), c)

    def struct_ref(self):
        return C.byref(self.struct)

    def nbytes(self):
        return self.kv.numel() * 4 + self.W.numel() * 4


def beam_search_table(table, out_vocab, num_beams, max_length, length_penalty, num_return_sequences=None, trie=None):
    """Device beam search driven by a logit table [B, max_length, Vd, Vd] — gdr_beam_search_table."""
    _need_cuda(table)
    table = _f32c(table)
    B = table.shape[0]
    nret = num_return_sequences or num_beams
    need = lib().gdr_beam_search_table_workspace_bytes(B, num_beams, max_length, out_vocab)
    ws = torch.empty(need, dtype=torch.uint8, device=table.device)
    ids = torch.empty((B * nret, max_length), dtype=torch.int64, device=table.device)
    lens = torch.empty((B * nret,), dtype=torch.int32, device=table.device)
    scores = torch.empty((B * nret,), dtype=torch.float64, device=table.device)
    check(lib().gdr_beam_search_table(ptr(table), B, out_vocab, num_beams, max_length, float(length_penalty), nret,
                                      trie.struct_ref() if trie is not None else None,
                                      ptr(ids), ptr(lens), ptr(scores), ptr(ws), ws.numel(), stream_ptr()),
          "gdr_beam_search_table")
    return ids, lens, scores


def finish_greedy_output(ids, lens):
    """Host tail of a num_beams = 1 call: _generate_no_beam_search returns input_ids as they stood when its loop ended
    (generation_utils.py:618-627), i.e. width = max(sent_lengths), which is what gdr_t5_generate leaves in out_len."""
    out = ids[:, :int(lens.max().item())].contiguous()
    _ffi.check_device_fault("generate")                      # the host has just synchronised: a faulted launch must not pass
    return out


def finish_generate_output(ids, lens, scores, max_length):
    """Host tail of generation_utils.py:905-919: width = min(max(len)+1, max_length); scores as Python floats."""
    sent_max_len = min(int(lens.max().item()) + 1, max_length)
    out = ids[:, :sent_max_len].contiguous(), scores.cpu().tolist()
    _ffi.check_device_fault("generate")                      # the host has just synchronised: a faulted launch must not pass
    return out
