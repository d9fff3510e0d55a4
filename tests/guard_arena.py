"""Guard-band arena: ONE uint8 allocation filled with a position-dependent pattern, out of which a test carves the tensors it hands to
libsgk.so. Everything that is not a carved view is guard, so a store in front of a buffer, behind it, or one whole outer slice (step, ring
slice, member, row) off lands on pattern bytes and check() reports it, where an exact-size torch tensor would have let it fall into the
caching allocator's rounding slack or a neighbour's block. Plain torch; importing needs no GPU.

    arena = Arena("cuda", "p")                      # or "~p", the bytewise complement: a stray byte cannot equal both
    out = arena.carve("actions", (n,), torch.uint8)
    w = arena.adopt("w1t", agent_w1t); arena.freeze("w1t")
    ... the call under test, a synchronize ...
    assert arena.check() == []

Pattern "p": byte i of the allocation is (i * 167 + 13) & 0xff (period 256, every residue once: 167 is odd).

Layout: views are 256-byte aligned (relative to the allocation's data_ptr AND absolutely: the base is checked). Every view has a guard of
at least max(4096, outer_bytes) bytes on EACH side that belongs to it alone; outer_bytes is the tensor's outermost stride (shape[1:]
elements) unless `outer` names another. Between two views lies nothing but the first one's after-guard, alignment padding (pattern too)
and the second one's before-guard. The last view's after-guard runs to the end of the allocation.

check() offsets: "before" counts from the view's first byte (the byte in front of it is -1), "after" from the first byte behind the view
(that byte is 0), "input" from the view's first byte.
"""
import torch

MIN_GUARD = 4096
ALIGN = 256
PATTERNS = ("p", "~p")


def pattern_bytes(pattern, start, stop, device="cpu"):
    """uint8 [stop - start]: what an untouched arena of `pattern` holds at allocation offsets start .. stop - 1."""
    if pattern not in PATTERNS:
        raise ValueError("pattern must be 'p' or '~p'")
    i = torch.arange(start, stop, dtype=torch.int64, device=device)
    b = ((i * 167 + 13) & 0xFF).to(torch.uint8)
    return b if pattern == "p" else b ^ 0xFF


def _nbytes(shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    return n


class Arena:
    def __init__(self, device, pattern, nbytes=1 << 20):
        if pattern not in PATTERNS:
            raise ValueError("pattern must be 'p' or '~p'")
        nbytes = (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN
        self.device, self.pattern, self.nbytes = torch.device(device), pattern, nbytes
        # ALIGN spare bytes so that offset 0 of the arena can be moved to a 256-byte boundary whatever the allocator hands out
        self._raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-self._raw.data_ptr()) % ALIGN
        self.buf = self._raw[skew:skew + nbytes]
        assert self.buf.data_ptr() % ALIGN == 0
        self._ref = pattern_bytes(pattern, 0, ALIGN, self.device).repeat(nbytes // ALIGN)  # what the guards must hold
        self.buf.copy_(self._ref)
        self._rec = {}  # name -> dict(start, end, guard, view, frozen)
        self._order = []
        self._cursor = 0  # first byte not yet spoken for (end of the last view's own after-guard)

    # ---- carving ------------------------------------------------------------------------------------------------------------------
    def carve(self, name, shape, dtype, fill=None, outer=None):
        """A contiguous view of `shape` / `dtype`; `outer` = bytes of the slowest dimension's stride when the shape does not show it
        (a flat tensor that the call treats as [slices][...]). Unfilled views keep the pattern: unwritten() then finds what a call
        that writes every entry left out. Raises ValueError when the arena has no room for the view AND both full guards."""
        if name in self._rec:
            raise ValueError("carved twice: %s" % name)
        shape = tuple(int(s) for s in shape)
        size = _nbytes(shape, dtype)
        outer_bytes = int(outer) if outer is not None else (_nbytes(shape[1:], dtype) if len(shape) > 1 else 0)
        guard = max(MIN_GUARD, outer_bytes)
        start = (self._cursor + guard + ALIGN - 1) // ALIGN * ALIGN
        end = start + size
        if end + guard > self.nbytes:
            raise ValueError("arena of %d bytes has no room for %s: view %d bytes + two guards of %d (next free byte %d)"
                             % (self.nbytes, name, size, guard, self._cursor))
        view = self.buf[start:end].view(dtype).view(shape)
        if fill is not None:
            view.fill_(fill)
        self._rec[name] = dict(start=start, end=end, guard=guard, lo=self._cursor, view=view, frozen=None, outer=outer_bytes)
        self._order.append(name)
        self._cursor = end + guard
        return view

    def adopt(self, name, tensor, outer=None):
        """Carve a view of the tensor's shape and dtype and copy the tensor in: param.data = arena.adopt("w1", param.data)."""
        view = self.carve(name, tensor.shape, tensor.dtype, outer=outer)
        view.copy_(tensor.detach().to(self.device))
        return view

    def freeze(self, name):
        """The view is an INPUT: check() reports any byte of it that changes from now on."""
        r = self._rec[name]
        r["frozen"] = self.buf[r["start"]:r["end"]].clone()

    # ---- layout facts the tests assert ----------------------------------------------------------------------------------------------
    def names(self):
        return list(self._order)

    def view(self, name):
        return self._rec[name]["view"]

    def span(self, name):
        """(start, end, guard, outer_bytes) in allocation offsets."""
        r = self._rec[name]
        return r["start"], r["end"], r["guard"], r["outer"]

    def layout_ok(self):
        """Every view aligned, with its own max(4096, outer) guard on both sides inside the allocation and clear of every other view."""
        prev_end = 0
        for n in self._order:
            r = self._rec[n]
            g = max(MIN_GUARD, r["outer"])
            if r["guard"] < g or r["start"] % ALIGN or r["view"].data_ptr() % ALIGN or not r["view"].is_contiguous():
                return False
            if r["start"] - g < prev_end or r["end"] + g > self.nbytes:  # prev_end already includes the neighbour's after-guard
                return False
            prev_end = r["end"] + g
        return True

    def guard_bytes(self):
        """How many pattern bytes check() compares."""
        return self.nbytes - sum(r["end"] - r["start"] for r in self._rec.values())

    # ---- the verdict ----------------------------------------------------------------------------------------------------------------
    def _regions(self):
        for k, n in enumerate(self._order):
            r = self._rec[n]
            hi = self.nbytes if k + 1 == len(self._order) else r["end"] + r["guard"]
            yield n, "before", r["lo"], r["start"], r["start"]
            yield n, "after", r["end"], hi, r["end"]
        if not self._order:
            yield "", "after", 0, self.nbytes, 0

    def check(self):
        """[(name, "before" | "after" | "input", first_offset, n_bytes)]: guard bytes that lost the pattern, frozen bytes that changed.
        The comparison runs on the device; a clean arena costs one scalar read-back."""
        bad = self.buf != self._ref
        for r in self._rec.values():
            seg = bad[r["start"]:r["end"]]
            if r["frozen"] is None:
                seg.zero_()
            else:
                torch.ne(self.buf[r["start"]:r["end"]], r["frozen"], out=seg)
        if not bool(bad.any()):
            return []
        out = []
        for name, side, lo, hi, origin in self._regions():
            idx = torch.nonzero(bad[lo:hi]).flatten()
            if idx.numel():
                out.append((name, side, int(idx[0]) + lo - origin, int(idx.numel())))
        for n in self._order:
            r = self._rec[n]
            if r["frozen"] is not None:
                idx = torch.nonzero(bad[r["start"]:r["end"]]).flatten()
                if idx.numel():
                    out.append((n, "input", int(idx[0]), int(idx.numel())))
        return out

    def unwritten(self, name):
        """How many aligned 4-byte groups of the view (the last group may be shorter) still hold the arena's pattern in every byte: 0 after
        a call that writes every entry. (Single bytes may equal the pattern by chance; four in a row of small integers or of a float
        cannot: consecutive pattern bytes differ by 167.)"""
        r = self._rec[name]
        same = self.buf[r["start"]:r["end"]] == self._ref[r["start"]:r["end"]]
        size = r["end"] - r["start"]
        if size == 0:
            return 0
        body = size // 4 * 4
        count = int(same[:body].view(-1, 4).all(dim=1).sum()) if body else 0
        if size > body:
            count += int(bool(same[body:].all()))
        return count
