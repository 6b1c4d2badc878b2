"""One byte arena per test case: every buffer of a library call is carved out of ONE uint8 tensor full of sentinel bytes, so that a store
outside a buffer the call may write lands on a byte a test looks at.

    a = Arena("cuda")
    a.input("ef", ef_numpy)                      # bytes copied in; must be bit-identical after the call
    a.output("ef_out", (R, E, oe), torch.float32)  # pre-filled with 0xFF bytes (NaN): an element the call never wrote is reported
    a.workspace("ws", nbytes)                    # exactly nbytes, pre-filled with a byte the case chooses
    a.build(ws_fill=0x00)
    rc = lib.gnx_...(a.ptr("ef"), ..., a.ptr("ws"), a.nbytes("ws"), ...)
    torch.cuda.synchronize()
    a.check()                                    # AssertionError naming carve, side, first and last offending offset

Layout: every carve starts ALIGN-byte aligned and has exactly the byte size it was declared with (a carve of 0 bytes is allowed: it has an
address and guards, and nothing may be written at it); at least GUARD sentinel bytes lie before the first carve, between two carves and
behind the last one.  `Arena(device, skew=f)` moves the start of carve c to its aligned start + f(c) bytes (even, below ALIGN, a multiple of
the carve's element size): the same buffers at addresses that are 256 k + 4, + 8, ... — a view into the middle of a tensor — with the same
guards (tests/test_gpu_alignment.py).  Plain torch: the same code checks CPU tensors (tests/test_arena_cpu.py proves that the checker can fail)."""
import numpy as np
import torch

GUARD = 64 * 1024  # a condition, not a measurement: a stray row or a whole stray tile still lands inside the arena
ALIGN = 256        # what torch's allocator gives every tensor, and where a carve starts without a skew; the ABI asks 4 bytes of fp32 and bf16
                   # buffers and 16 of a workspace (include/gnx.h), which Arena(skew=...) places a carve at
SENTINEL = 0xA5
UNWRITTEN = 0xFF   # fp32 0xFFFFFFFF and bf16 0xFFFF are NaNs

INPUT, OUTPUT, WORKSPACE = "input", "output", "workspace"


class Carve:
    __slots__ = ("name", "kind", "nbytes", "off", "data", "dtype", "shape")

    def __init__(self, name, kind, nbytes, data=None, dtype=None, shape=None):
        self.name, self.kind, self.nbytes, self.off, self.data, self.dtype, self.shape = name, kind, int(nbytes), None, data, dtype, shape


def _bytes_of(data):
    """the bytes of a numpy array / torch tensor as a CPU uint8 tensor"""
    if isinstance(data, torch.Tensor):
        t = data.detach().contiguous().cpu()
        return t.view(-1).view(torch.uint8).clone() if t.numel() else torch.empty(0, dtype=torch.uint8)
    a = np.ascontiguousarray(data)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()) if a.size else torch.empty(0, dtype=torch.uint8)


class Arena:
    def __init__(self, device="cpu", guard=GUARD, skew=None):
        """`skew`: None, or a callable (Carve) -> bytes by which the carve starts behind its ALIGN-aligned start"""
        self.device, self.guard, self.skew = torch.device(device), int(guard), skew
        self.carves, self.by_name, self.buf, self.snap, self.queries = [], {}, None, None, []

    # ---- declaration ----
    def _add(self, c):
        assert self.buf is None, "the arena is already built"
        assert c.name not in self.by_name, c.name
        assert c.nbytes >= 0
        self.carves.append(c)
        self.by_name[c.name] = c
        return c.name

    def input(self, name, data):
        """a buffer the call only reads: a numpy array or torch tensor whose bytes are copied in (dtype and shape are kept for view())"""
        b = _bytes_of(data)
        dtype = data.dtype if isinstance(data, torch.Tensor) else torch.from_numpy(np.zeros(0, dtype=np.asarray(data).dtype)).dtype
        return self._add(Carve(name, INPUT, b.numel(), b, dtype, tuple(data.shape)))

    def output(self, name, shape, dtype=torch.float32):
        shape = tuple(int(v) for v in shape)
        return self._add(Carve(name, OUTPUT, int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size(), None, dtype, shape))

    def workspace(self, name, nbytes):
        """`nbytes`: the value of the *_workspace_bytes query — or a callable returning it, for a query whose descriptor needs the addresses of
        other carves (weights): build() lays the arena out once with such workspaces empty, calls it, and lays the arena out again (the
        addresses move; a size query does not depend on their values)"""
        if callable(nbytes):
            c = Carve(name, WORKSPACE, 0, nbytes, torch.uint8, (0,))
            return self._add(c)
        return self._add(Carve(name, WORKSPACE, nbytes, None, torch.uint8, (int(nbytes),)))

    def _skew_of(self, c):
        if self.skew is None:
            return 0
        k = int(self.skew(c))
        assert 0 <= k < ALIGN and k % 2 == 0, (c.name, k)
        assert k % torch.empty(0, dtype=c.dtype).element_size() == 0, (c.name, k, c.dtype)
        return k

    # ---- build / refill ----
    def build(self, ws_fill=0x00):
        late = [c for c in self.carves if c.kind == WORKSPACE and callable(c.data)]
        if late:
            queries = self.queries = [(c, c.data) for c in late]
            for c in late:
                c.data = None
            self.build(ws_fill)  # provisional: the late workspaces have no bytes yet
            for c, q in queries:
                c.nbytes = int(q())
                assert c.nbytes >= 0
                c.shape = (c.nbytes,)
            self.buf = self.snap = None
        off = 0
        for c in self.carves:
            off = (off + self.guard + ALIGN - 1) // ALIGN * ALIGN + self._skew_of(c)
            c.off = off
            off += c.nbytes
        total = off + self.guard
        store = torch.full((total + ALIGN,), SENTINEL, dtype=torch.uint8, device=self.device)
        skip = -store.data_ptr() % ALIGN  # (a CPU allocation is 64-byte aligned: start at the next multiple of ALIGN)
        self.buf = store[skip:skip + total]
        assert self.buf.data_ptr() % ALIGN == 0
        for c in self.carves:
            if c.kind == INPUT and c.nbytes:
                self.buf[c.off:c.off + c.nbytes] = c.data.to(self.device)  # (the declared bytes stay in c.data: every layout starts from them)
        self.refill(ws_fill)
        self.snap = self.buf.clone()
        return self

    def relayout(self, skew, ws_fill=0x00):
        """the same carves laid out again under another skew (None: aligned): what build() would have given had the arena been declared with
        it.  The inputs are filled from the bytes they were DECLARED with, not from the previous layout — a call that corrupted an input there is
        reported there and nowhere else.  The workspace queries run again, at the new addresses."""
        assert self.buf is not None
        for c, q in self.queries:
            c.data, c.nbytes, c.shape = q, 0, (0,)
        self.skew, self.buf, self.snap = skew, None, None
        return self.build(ws_fill)

    def refill(self, ws_fill):
        """outputs back to 0xFF bytes, every workspace to `ws_fill` — the state before a call (inputs and guards are left as they are: a call
        that changed them has been reported by check())"""
        for c in self.carves:
            if c.nbytes and c.kind == OUTPUT:
                self.buf[c.off:c.off + c.nbytes] = UNWRITTEN
            elif c.nbytes and c.kind == WORKSPACE:
                self.buf[c.off:c.off + c.nbytes] = int(ws_fill)

    # ---- access ----
    def nbytes(self, name):
        return self.by_name[name].nbytes

    def ptr(self, name):
        """device address of a carve (None for a name of None: `nothing`)"""
        if name is None:
            return None
        return self.buf.data_ptr() + self.by_name[name].off

    def raw(self, name):
        c = self.by_name[name]
        return self.buf[c.off:c.off + c.nbytes]

    def view(self, name):
        """the carve as a tensor of its declared dtype and shape (shares the arena's memory)"""
        c = self.by_name[name]
        if c.nbytes == 0:
            return torch.empty(c.shape, dtype=c.dtype, device=self.device)
        return self.raw(name).view(c.dtype).view(c.shape)

    def numpy(self, name):
        t = self.view(name)
        return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()

    def output_bits(self):
        """{name: a copy of the bytes} of every output carve: what two runs of a case must agree on bit for bit"""
        return {c.name: self.raw(c.name).clone() for c in self.carves if c.kind == OUTPUT}

    # ---- the check ----
    def violations(self, unwritten=True):
        """A list of findings (strings), empty when the call kept the contract: every byte outside an output or workspace carve is what it
        was at build() — guards still sentinel, inputs equal to their snapshot — and (`unwritten`) no element of an output still holds the
        0xFF bytes it was given."""
        assert self.buf is not None
        diff = self.buf != self.snap
        for c in self.carves:
            if c.kind != INPUT and c.nbytes:
                diff[c.off:c.off + c.nbytes] = False
        found = []
        if bool(diff.any()):
            idx = diff.nonzero().view(-1).cpu().numpy()
            starts = np.array([c.off for c in self.carves], dtype=np.int64)
            ends = np.array([c.off + c.nbytes for c in self.carves], dtype=np.int64)
            # the carve a byte belongs to: inside an input, else the nearer of the carve that ends before it and the carve that starts after it
            far = np.iinfo(np.int64).max
            k = np.searchsorted(starts, idx, side="right") - 1  # last carve starting at or before the byte (-1: none)
            kp, kn = np.clip(k, 0, None), np.clip(k + 1, None, len(starts) - 1)
            inside = (k >= 0) & (idx < ends[kp])
            d_prev = np.where(k >= 0, idx - ends[kp] + 1, far)             # bytes past the end of carve k (1 = the byte just behind it)
            d_next = np.where(k + 1 < len(starts), starts[kn] - idx, far)  # bytes in front of carve k + 1 (1 = the byte just before it)
            after = ~inside & (d_prev <= d_next)
            key = np.where(inside | after, k, k + 1) * 3 + np.where(inside, 0, np.where(after, 2, 1))
            for u in np.unique(key).tolist():
                offs = idx[key == u].tolist()
                side = ("inside", "before", "after")[u % 3]
                c = self.carves[u // 3]
                rel = (lambda o: o - c.off) if side == "inside" else ((lambda o: o - (c.off + c.nbytes)) if side == "after" else (lambda o: o - c.off))
                what = {"inside": f"{c.kind} '{c.name}' was modified", "after": f"write AFTER {c.kind} '{c.name}' ({c.nbytes} bytes)",
                        "before": f"write BEFORE {c.kind} '{c.name}' ({c.nbytes} bytes)"}[side]
                ref = "its end" if side == "after" else "its start"
                found.append(f"{what}: {len(offs)} bytes, first at {rel(offs[0]):+d} and last at {rel(offs[-1]):+d} from {ref} "
                             f"(arena offsets {offs[0]}..{offs[-1]})")
        if unwritten:
            for c in self.carves:
                if c.kind != OUTPUT or c.nbytes == 0:
                    continue
                es = torch.empty(0, dtype=c.dtype).element_size()
                still = (self.raw(c.name).view(-1, es) == UNWRITTEN).all(dim=1)
                if bool(still.any()):
                    w = still.nonzero().view(-1)
                    found.append(f"output '{c.name}' {c.shape}: {int(w.numel())} of {int(still.numel())} elements never written, "
                                 f"first element {int(w[0])}, last {int(w[-1])}")
        return found

    def check(self, what="", unwritten=True):
        found = self.violations(unwritten)
        assert not found, (what + ": " if what else "") + "; ".join(found)
