"""Run host code under fenced, poisoned allocations: the memory contract between the Python layer and the kernels.

No ``.hip`` file allocates; every device buffer a kernel touches is a ``torch.empty`` / ``empty_like`` / ``zeros`` /
``zeros_like`` / ``full`` / ``Tensor.new_empty`` / ``Tensor.new_zeros`` of the Python layer.  ``fenced()`` replaces those
seven names while it is active (and restores them on exit, also on error, the way ``relu_margins`` in conftest.py
patches ``torch.relu``).  A contiguous allocation on a listed device becomes one ``uint8`` base buffer

    [ fence, 64 KiB | payload, padded to a multiple of 512 B | fence, 64 KiB ]

and the caller gets the payload with the shape and dtype it asked for (a tensor on the base's storage at an offset; not
an autograd view, so in-place work on it behaves as on a tensor of its own).

* FENCE is 64 KiB: a condition, not a measurement.  An overrun by one whole ragged tile (16 rows x 64 floats = 4 KiB) or
  by one scratch slab stays inside memory the run owns.  It is a multiple of 512 B, and the caching allocator hands out
  512-byte-aligned blocks, so the payload sits at the same address modulo 512 as in production and the kernels that
  choose a 16-byte route from pointer alignment choose the same one.
* fences hold the byte FENCE_BYTE, and so does the padding behind the payload (it belongs to the upper fence: an overrun
  into the allocator's rounding is the silent kind); ``check()`` asserts that every one of those bytes still does.
* floating payloads of ``empty*`` hold a quiet NaN of ONE fixed bit pattern (fp32 0x7FC5A5A5): a computed NaN and a word
  nobody wrote can be told apart, and the existing oracles (``assert_matches`` rejects non-finite values, ``torch.equal``
  rejects NaN) fail on a returned word that was never written.
* ``zeros*`` / ``full`` payloads keep their value and are fenced.
* INTEGER, BOOL AND BYTE payloads of ``empty*`` are filled with ZERO, not with poison.  A poisoned index, read by a
  kernel because another kernel failed to write it, is a wild address, and a GPU fault on a shared machine must not be
  provoked.  Index outputs that are not written remain the job of the bit-exact plan tests.
* every base stays alive until the block ends, so nothing is recycled inside one run (and so a use-after-free is NOT
  seen: see DESIGN.md).
* passed through to the real function, and counted per category in ``passed``: tensors on a device that is not listed
  (``cpu``), ``pin_memory``, an explicit ``memory_format``, a non-contiguous ``empty_like`` / ``zeros_like``, and
  anything allocated while the current stream is capturing (``capture``: the fills would become graph nodes).  Whatever
  else the shim does not understand is counted as ``other`` with its site in ``other_sites``; a test asserts it is empty.

``check()`` runs on a clean exit after ``torch.cuda.synchronize()``; its message names each breached allocation by site,
side and offset of the first damaged byte, and lists the sites whose payloads still hold exact-poison words (diagnosis,
not an assertion: scratch may be over-sized).  ``unwritten(t)`` counts the exact-poison words of one tensor.
``records`` holds (base, payload bytes, site, payload, poisoned) per allocation; ``sites`` the set of call sites.
"""
import os
import sys

import torch

FENCE = 64 * 1024            # bytes on each side; never lowered (device memory has not forced it)
FENCE_BYTE = 0xA5
ROUND = 512                  # the caching allocator's block granularity
# one quiet NaN per float width: sign 0, exponent all ones, the quiet bit, and a payload no arithmetic produces
POISON = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float64: (torch.int64, 0x7FF8A5A5C5A5A5A5),
          torch.float16: (torch.int16, 0x7E5A), torch.bfloat16: (torch.int16, 0x7FC5)}
PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "full", "new_empty", "new_zeros")
_HERE = os.path.abspath(__file__)
_ROOT = os.path.dirname(os.path.dirname(_HERE))


def _site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    name = os.path.abspath(f.f_code.co_filename)
    if name.startswith(_ROOT + os.sep):
        name = os.path.relpath(name, _ROOT)
    return f"{name}:{f.f_lineno}"


def _size(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = args[0]
    return tuple(int(s) for s in args)


def unwritten(t):
    """Number of words of ``t`` that still hold the exact poison pattern of its dtype (0 for non-float tensors)."""
    if t.dtype not in POISON or t.numel() == 0:
        return 0
    as_int, pattern = POISON[t.dtype]
    return int((t.detach().contiguous().view(as_int) == pattern).sum())


class fenced:
    def __init__(self, devices=("cuda",)):
        self.devices = tuple(devices)
        self.records = []                     # (base, payload bytes, site, payload tensor, poisoned)
        self.passed = {"device": 0, "pin_memory": 0, "memory_format": 0, "non_contiguous": 0, "capture": 0, "other": 0}
        self.other_sites = []
        self._saved = None

    # ------------------------------------------------------------------------------------------- allocation
    def _device(self, device):
        if device is None:
            return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
        return torch.device(device)

    def _pass(self, why, dev):
        """Count a pass-through (``device``: any; the other categories are of allocations on a listed device by construction)."""
        self.passed[why] += 1
        if why == "other":
            self.other_sites.append(_site())

    def _route(self, dev, kw):
        """None to fence, else the category under which the call is passed through."""
        if dev.type not in self.devices:
            return "device"
        if kw.get("pin_memory"):
            return "pin_memory"
        if kw.get("memory_format") is not None:
            return "memory_format"
        if kw.get("layout", torch.strided) is not torch.strided or kw.get("out") is not None or kw.get("names") is not None:
            return "other"
        if set(kw) - {"pin_memory", "memory_format", "layout", "out", "names", "requires_grad"}:
            return "other"
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return "capture"
        return None

    def _alloc(self, shape, dtype, dev, fill, site, requires_grad=False):
        """fill: None = empty (poison floats, zero the rest), else the value the payload is to hold."""
        o = self._saved
        item = dtype.itemsize
        n = 1
        for s in shape:
            n *= s
        nbytes = n * item
        padded = -(-nbytes // ROUND) * ROUND
        base = o["empty"](FENCE + padded + FENCE, dtype=torch.uint8, device=dev)
        base.fill_(FENCE_BYTE)
        stride, acc = [], 1
        for s in reversed(shape):
            stride.append(acc)
            acc *= max(s, 1)
        pay = o["empty"](0, dtype=dtype, device=dev).set_(base.untyped_storage(), base.storage_offset() + FENCE // item,
                                                           shape, tuple(reversed(stride)))
        poisoned = False
        if fill is not None:
            pay.fill_(fill)
        elif dtype in POISON:
            as_int, pattern = POISON[dtype]
            pay.view(as_int).fill_(pattern)
            poisoned = True
        elif dtype.is_complex:
            pay.fill_(complex(float("nan"), float("nan")))
        else:
            pay.zero_()
        self.records.append((base, nbytes, site, pay, poisoned))
        if requires_grad:
            pay.requires_grad_(True)
        return pay

    # ------------------------------------------------------------------------------------------- the patched names
    def _make(self):
        o = self._saved

        def sized(name, fill):
            def f(*size, dtype=None, device=None, **kw):
                dev = self._device(device)
                why = self._route(dev, kw)
                if why is not None:
                    self._pass(why, dev)
                    return o[name](*size, dtype=dtype, device=device, **kw)
                return self._alloc(_size(size), dtype or torch.get_default_dtype(), dev, fill, _site(),
                                   kw.get("requires_grad", False))
            f.__name__ = name
            return f

        def like(name, fill):
            def f(t, dtype=None, device=None, **kw):
                dev = self._device(device) if device is not None else t.device
                why = self._route(dev, kw)
                if why is None and not t.is_contiguous():
                    why = "non_contiguous"
                if why is not None:
                    self._pass(why, dev)
                    return o[name](t, dtype=dtype, device=device, **kw)
                return self._alloc(tuple(t.shape), dtype or t.dtype, dev, fill, _site(), kw.get("requires_grad", False))
            f.__name__ = name
            return f

        def new(name, fill):
            def f(t, *size, dtype=None, device=None, **kw):
                dev = self._device(device) if device is not None else t.device
                why = self._route(dev, kw)
                if why is not None:
                    self._pass(why, dev)
                    return o[name](t, *size, dtype=dtype, device=device, **kw)
                return self._alloc(_size(size), dtype or t.dtype, dev, fill, _site(), kw.get("requires_grad", False))
            f.__name__ = name
            return f

        def full(size, fill_value, dtype=None, device=None, **kw):
            dev = self._device(device)
            why = self._route(dev, kw)
            if why is None and isinstance(fill_value, torch.Tensor):
                why = "other"
            if why is not None:
                self._pass(why, dev)
                return o["full"](size, fill_value, dtype=dtype, device=device, **kw)
            if dtype is None:
                dtype = (torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int)
                         else torch.get_default_dtype())
            return self._alloc(_size((size,)), dtype, dev, fill_value, _site(), kw.get("requires_grad", False))

        return {"empty": sized("empty", None), "zeros": sized("zeros", 0), "empty_like": like("empty_like", None),
                "zeros_like": like("zeros_like", 0), "full": full, "new_empty": new("new_empty", None),
                "new_zeros": new("new_zeros", 0)}

    def __enter__(self):
        self._saved = {n: getattr(torch.Tensor if n.startswith("new_") else torch, n) for n in PATCHED}
        self._own = {n: n in torch.Tensor.__dict__ for n in PATCHED if n.startswith("new_")}
        for n, f in self._make().items():
            setattr(torch.Tensor if n.startswith("new_") else torch, n, f)
        return self

    def __exit__(self, *exc):
        for n, f in self._saved.items():
            if not n.startswith("new_"):
                setattr(torch, n, f)
            elif self._own[n]:
                setattr(torch.Tensor, n, f)
            else:
                delattr(torch.Tensor, n)          # inherited from the C base class: take our override away again
        try:
            if exc[0] is None:
                self.check()
        finally:
            self.records =[(None, r[1], r[2], None, r[4]) for r in self.records]      # let the arena go
        return False

    # ------------------------------------------------------------------------------------------- the checks
    @property
    def sites(self):
        """The call sites (``file:line``, relative to the repository) of every fenced allocation so far."""
        return {r[2] for r in self.records}

    def breaches(self):
        """[(site, side, offset of the first damaged byte within that fence)] over every allocation."""
        live = [r for r in self.records if r[0] is not None]
        if not live:
            return []
        if any(r[0].is_cuda for r in live):
            torch.cuda.synchronize()
        flags = [torch.stack([(r[0][:FENCE] != FENCE_BYTE).any(), (r[0][FENCE + r[1]:] != FENCE_BYTE).any()]) for r in live]
        flags = torch.stack([f.cpu() for f in flags])        # every comparison is queued before the first copy waits
        out = []
        for (base, nbytes, site, _, _), (lo, hi) in zip(live, flags.tolist()):
            for side, hit, fence in (("below", lo, base[:FENCE]), ("above", hi, base[FENCE + nbytes:])):
                if hit:
                    out.append((site, side, int((fence != FENCE_BYTE).nonzero()[0])))
        return out

    def poisoned_sites(self):
        """{site: exact-poison words left in its payloads}: diagnosis (scratch may be over-sized), not an assertion."""
        live = [r for r in self.records if r[0] is not None and r[4] and r[1]]
        if not live:
            return {}
        counts = [(r[3].detach().view(POISON[r[3].dtype][0]) == POISON[r[3].dtype][1]).sum() for r in live]
        out = {}
        for r, c in zip(live, [int(c) for c in torch.stack([c.cpu() for c in counts]).tolist()]):
            if c:
                out[r[2]] = out.get(r[2], 0) + c
        return out

    def check(self):
        bad = self.breaches()
        if bad:
            left = self.poisoned_sites()
            lines = [f"  {site}: fence {side} the payload, first damaged byte at offset {off}" for site, side, off in bad]
            lines += [f"  (never written: {n} word(s) of the payloads from {site})" for site, n in sorted(left.items())]
            raise AssertionError("fence breached:\n" + "\n".join(lines))
