"""Guard bands, poisoned scratch and tailed inputs for the tests of the C ABI's memory contract (include/gdr_hip.h).

The GPU has no address sanitizer this project may use, so a stray store or load is made visible by where the buffers sit:

  * guarded(shape, dtype, device): the tensor a kernel writes lives inside ONE flat uint8 allocation that is filled with a
    fixed byte pattern; the returned view starts 256-byte aligned, at least BEFORE_MIN bytes after the allocation's start,
    and is followed by at least max(AFTER_MIN, 256 rows of the tensor) pattern bytes.  handle.check() compares both bands
    with the pattern byte for byte, on the device.  The logical region starts out holding the pattern too, so the pad
    columns of a strided output (a [M, ld] guarded tensor of which a kernel may write [:, :N]) can be checked with
    handle.check_columns(N).
  * guarded_input(tensor, tail=...): an input with caller-chosen content directly behind its last element (rows that would
    win a top-k, NaN rows, valid token ids ...); handle.unchanged() asserts the call did not modify the logical region or
    the tail.
  * poisoned_workspace(nbytes, fill): a guarded scratch buffer of EXACTLY nbytes filled with `fill`: the band starts at
    the first byte past what a *_workspace_bytes function returned.

The band sizes are conditions of the check, not measurements: a kernel that stores a whole tile row or column too many lands
inside them."""
import torch

BEFORE_MIN = 64 << 10
AFTER_MIN = 1 << 20
ALIGN = 256
_PERIOD = 251                      # prime: a block of pattern copied to a shifted position does not match


def _pattern(a, b, device):
    """Pattern bytes of positions [a, b) of an allocation: 1 + (i mod 251) — never zero, never 0xFF, position dependent."""
    one = (torch.arange(_PERIOD, device=device, dtype=torch.int16) + 1).to(torch.uint8).roll(-(a % _PERIOD))
    return one.repeat(-(-(b - a) // _PERIOD))[:b - a]


class Guard:
    def __init__(self, flat, lo, nbytes, view):
        self.flat, self.lo, self.nbytes, self.view = flat, lo, nbytes, view
        self._snapshot = None

    # ---- bands
    def _bad(self, a, b, what):
        expect = _pattern(a, b, self.flat.device)
        got = self.flat[a:b]
        if torch.equal(got, expect):
            return None
        where = torch.nonzero(got != expect).flatten()
        first, last, n = int(where[0]), int(where[-1]), int(where.numel())
        rel = (first - (b - a), last - (b - a)) if what == "before" else (first, last)
        return f"{n} bytes of the band {what} the buffer were overwritten (first at {rel[0]:+d}, last at {rel[1]:+d} bytes from the buffer's {'start' if what == 'before' else 'end'})"

    def check(self, what="buffer"):
        """Both bands still hold the pattern (compared on the device, byte for byte)."""
        torch.cuda.synchronize(self.flat.device)
        for msg in (self._bad(0, self.lo, "before"), self._bad(self.lo + self.nbytes, self.flat.numel(), "after")):
            assert msg is None, f"{what}: {msg}"

    def check_columns(self, n_cols, what="buffer"):
        """For a 2-D view [rows, ld] of which the call may write [:, :n_cols]: columns n_cols.. still hold the pattern."""
        torch.cuda.synchronize(self.flat.device)
        assert self.view.dim() == 2
        esz = self.view.element_size()
        rows, ld = self.view.shape
        expect = _pattern(self.lo, self.lo + self.nbytes, self.flat.device).view(rows, ld * esz)
        got = self.flat[self.lo:self.lo + self.nbytes].view(rows, ld * esz)
        bad = got[:, n_cols * esz:] != expect[:, n_cols * esz:]
        if bool(bad.any()):
            r, c = [int(x) for x in torch.nonzero(bad)[0]]
            raise AssertionError(f"{what}: pad columns written — {int(bad.sum())} bytes, first at row {r}, column {n_cols + c // esz}")

    # ---- inputs
    def snapshot(self):
        self._snapshot = self.flat.clone()
        return self

    def unchanged(self, what="input"):
        """The whole allocation (logical region, tail and bands) is what it was when snapshot() was taken."""
        torch.cuda.synchronize(self.flat.device)
        assert self._snapshot is not None, "snapshot() was never taken"
        if not torch.equal(self.flat, self._snapshot):
            where = torch.nonzero(self.flat != self._snapshot).flatten()
            raise AssertionError(f"{what}: modified by the call — {int(where.numel())} bytes, first at {int(where[0]) - self.lo:+d} "
                                 "bytes from the tensor's start")


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def guarded(shape, dtype, device, before=BEFORE_MIN, after=AFTER_MIN):
    """(view, handle): a tensor of `shape` / `dtype` inside a pattern-filled allocation.  before / after are lower bounds of the
    band sizes in bytes; they are raised to the module's minima and, for `after`, to 256 rows of the tensor."""
    shape = tuple(int(s) for s in shape)
    esz = torch.empty((), dtype=dtype).element_size()
    nbytes = _numel(shape) * esz
    row = (shape[-1] if len(shape) >= 2 else 1) * esz              # a 1-D tensor is one row per element
    before = -(-max(int(before), BEFORE_MIN) // ALIGN) * ALIGN
    after = max(int(after), AFTER_MIN, 256 * row)
    flat = torch.empty(before + ALIGN + nbytes + after, dtype=torch.uint8, device=device)
    lo = before + (-(flat.data_ptr() + before)) % ALIGN
    flat.copy_(_pattern(0, flat.numel(), device))
    view = flat[lo:lo + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % ALIGN == 0 and lo >= BEFORE_MIN and flat.numel() - lo - nbytes >= after
    return view, Guard(flat, lo, nbytes, view)


def guarded_input(tensor, tail=None):
    """(view, handle): a copy of `tensor` (any device) inside a guarded allocation on the GPU, followed IMMEDIATELY by `tail` (a
    tensor of the same dtype whose meaning the caller chooses: what a kernel would pick up if it read past the logical end).
    The snapshot is taken: handle.unchanged() holds as long as nothing writes the allocation."""
    assert tensor.is_contiguous()
    dev = tensor.device if tensor.is_cuda else torch.device("cuda:0")
    n_tail = 0 if tail is None else tail.numel()
    row_bytes = (tensor.shape[-1] if tensor.dim() >= 2 else 1) * tensor.element_size()
    flat_view, h = guarded((tensor.numel() + n_tail,), tensor.dtype, dev, after=256 * row_bytes)
    flat_view[:tensor.numel()].copy_(tensor.reshape(-1))
    if n_tail:
        assert tail.dtype == tensor.dtype and tail.is_contiguous()
        flat_view[tensor.numel():].copy_(tail.reshape(-1))
    h.view = flat_view[:tensor.numel()].view(tensor.shape)
    h.snapshot()
    return h.view, h


def poisoned_workspace(nbytes, fill, device):
    """(uint8 view of exactly nbytes filled with `fill`, handle); nbytes == 0 gives (None, None): the NULL workspace."""
    if nbytes == 0:
        return None, None
    view, h = guarded((int(nbytes),), torch.uint8, device)
    view.fill_(int(fill))
    return view, h
