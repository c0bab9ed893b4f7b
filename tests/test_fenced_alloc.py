"""The fenced-allocation shim of tests/fenced.py can fail: on CPU tensors (no GPU needed) it detects a word written past
either end of a payload and names the site and the side, counts the words nobody wrote, leaves ``zeros`` zero, counts
what it passes through and restores the patched names after an error.  One ``gpu`` case repeats the detection on device
memory.  Every stray write here is plain torch indexing into memory the test owns."""
import pytest
import torch

import fenced as F
from fenced import fenced, unwritten

ME = "tests/test_fenced_alloc.py"


class _Square(torch.autograd.Function):
    """An op shaped like the package's: the output and a scratch buffer allocated inside, scratch saved for backward."""

    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        s = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
        torch.mul(x, x, out=y)
        s.copy_(x.reshape(-1))
        ctx.save_for_backward(s)
        return y

    @staticmethod
    def backward(ctx, dy):
        s, = ctx.saved_tensors
        dx = dy.new_empty(dy.shape)
        torch.mul(dy, 2 * s.view_as(dy), out=dx)
        return dx


def _originals():
    return [getattr(torch, n) for n in F.PATCHED if not n.startswith("new_")] + \
           [torch.Tensor.new_empty, torch.Tensor.new_zeros, "new_empty" in torch.Tensor.__dict__]


def test_autograd_function_gives_correct_gradients_under_the_shim():
    x = torch.randn(5, 7, requires_grad=True)
    with fenced(("cpu",)) as f:
        y = _Square.apply(x)
        g, = torch.autograd.grad((y * torch.arange(35.0).view(5, 7)).sum(), x)
        assert len(f.records) >= 3 and y.data_ptr() % 512 == f.records[0][0].data_ptr() % 512
        assert unwritten(y) == 0 and unwritten(g) == 0
    assert torch.equal(y, x.detach() * x.detach())
    assert torch.allclose(g, 2 * x.detach() * torch.arange(35.0).view(5, 7))
    assert {s.split(":")[0] for s in f.sites} == {ME}


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("kind", ["empty", "zeros", "new_empty"])
def test_one_word_past_either_end_is_caught_and_named(kind, side):
    with pytest.raises(AssertionError) as err:
        with fenced(("cpu",)) as f:
            other = torch.empty(3, 5, dtype=torch.float32, device="cpu")
            other.fill_(1.0)
            if kind == "new_empty":
                t = other.new_empty(10)
            else:
                t = getattr(torch, kind)(10, dtype=torch.float32, device="cpu")       # the site check() must name
            t.fill_(2.0)
            base, nbytes = f.records[-1][0], f.records[-1][1]
            assert nbytes == 40 and f.records[-1][3] is t
            word = base.view(torch.float32)
            at = F.FENCE // 4 - 1 if side == "below" else F.FENCE // 4 + 10
            word[at] = 3.0                                                             # one word outside the payload
    text = str(err.value)
    line = [ln for ln in text.splitlines() if "fence " in ln and ME in ln]
    assert len(line) == 1 and f"fence {side}" in line[0], text
    # the site is the line of the allocation of ``t``, not of ``other``, and the offset is that of the damaged word
    import inspect
    src, first = inspect.getsourcelines(test_one_word_past_either_end_is_caught_and_named)
    want = first + next(i for i, ln in enumerate(src) if ("other.new_empty" if kind == "new_empty" else "getattr(torch, kind)") in ln)
    assert f"{ME}:{want}:" in line[0], (line[0], want)
    off = F.FENCE - 4 if side == "below" else 0
    assert line[0].endswith(f"offset {off}"), line[0]


def test_overrun_into_the_padding_counts_as_a_breach():
    """The 512-byte rounding belongs to the fence: a word just past a 40-byte payload is damage, as it would be silent
    in the caching allocator's rounding."""
    with fenced(("cpu",)) as f:
        torch.empty(10, dtype=torch.float32, device="cpu").zero_()
        f.records[-1][0][F.FENCE + 40] = 0
        assert f.breaches() == [(f.records[-1][2], "above", 0)]
        f.records[-1][0][F.FENCE + 40] = F.FENCE_BYTE
        assert f.breaches() == []


def test_partly_written_empty_reports_the_exact_count():
    with fenced(("cpu",)) as f:
        t = torch.empty(3, 4, dtype=torch.float32, device="cpu")
        assert unwritten(t) == 12 and bool(torch.isnan(t).all())
        t[0] = 1.0
        t[2, 3] = float("nan")                       # a computed NaN is not the poison
        assert unwritten(t) == 7
        assert f.poisoned_sites() == {f.records[-1][2]: 7}
        for dt in (torch.float64, torch.float16, torch.bfloat16):
            h = torch.empty(5, dtype=dt, device="cpu")
            assert unwritten(h) == 5 and bool(torch.isnan(h).all())
            h[1:3] = 0
            assert unwritten(h) == 3
        i = torch.empty(6, dtype=torch.int64, device="cpu")
        assert unwritten(i) == 0 and not bool(i.any())        # integer payloads are zero, not poison
        b = torch.empty(6, dtype=torch.uint8, device="cpu")
        assert not bool(b.any())


def test_zeros_and_full_keep_their_value_and_are_fenced():
    with fenced(("cpu",)) as f:
        z = torch.zeros(7, 3, device="cpu")
        zl = torch.zeros_like(z)
        nz = z.new_zeros(4, dtype=torch.int32)
        fl = torch.full((5,), -1, dtype=torch.int64, device="cpu")
        assert len(f.records) == 4
        assert not bool(z.any()) and not bool(zl.any()) and not bool(nz.any()) and bool((fl == -1).all())
        assert z.shape == (7, 3) and nz.dtype == torch.int32 and zl.is_contiguous()
        assert all(bool((r[0][:F.FENCE] == F.FENCE_BYTE).all()) and bool((r[0][-F.FENCE:] == F.FENCE_BYTE).all())
                   for r in f.records)
        assert torch.empty(0, device="cpu").numel() == 0 and torch.zeros((), device="cpu").dim() == 0


def test_pass_through_cases_are_counted():
    with fenced(("cuda",)) as f:                      # cpu is not listed: everything below is the real function's
        torch.empty(4, device="cpu")
        torch.zeros(4)
        assert f.passed["device"] == 2 and not f.records
    with fenced(("cpu",)) as f:
        nc = torch.empty(6, 4, device="cpu").t()
        assert not nc.is_contiguous()
        a = torch.empty_like(nc)
        b = torch.zeros_like(torch.empty(4, device="cpu"), memory_format=torch.preserve_format)
        c = torch.empty(2, 3, 4, 5, device="cpu", memory_format=torch.channels_last)
        d = torch.empty(3, device="cpu", layout=torch.sparse_coo)
        assert a.shape == (4, 6) and b.shape == (4,) and c.shape == (2, 3, 4, 5) and d.layout is torch.sparse_coo
        assert len(f.records) == 2                   # the two contiguous empties above
        assert f.passed == {"device": 0, "pin_memory": 0, "memory_format": 2, "non_contiguous": 1, "capture": 0,
                            "other": 1}
        assert len(f.other_sites) == 1 and f.other_sites[0].startswith(ME)


def test_names_are_restored_after_an_exception():
    before = _originals()
    with pytest.raises(RuntimeError, match="inside"):
        with fenced(("cpu",)):
            assert _originals()[:-1] != before[:-1]
            raise RuntimeError("inside")
    assert _originals() == before
    with pytest.raises(AssertionError, match="fence breached"):
        with fenced(("cpu",)) as f:
            torch.empty(1, device="cpu")
            f.records[0][0][0] = 0
    assert _originals() == before
    assert torch.empty(3).untyped_storage().nbytes() < F.FENCE       # the real one again


@pytest.mark.gpu
def test_overrun_and_unwritten_words_are_detected_on_device_memory():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    with pytest.raises(AssertionError) as err:
        with fenced() as f:
            t = torch.empty(33, 7, dtype=torch.float32, device="cuda")
            z = torch.zeros_like(t)
            assert t.data_ptr() % 512 == 0 and t.is_contiguous() and unwritten(t) == 231 and unwritten(z) == 0
            t[:30] = 1.0
            assert unwritten(t) == 21
            assert f.breaches() == []
            f.records[1][0].view(torch.float32)[F.FENCE // 4 + 231] = 1.0          # one word past the end of z
    text = str(err.value)
    assert "fence above" in text and "offset 0" in text and text.count("fence above") + text.count("fence below") == 1, text
    assert "never written: 21 word(s)" in text, text
    assert f.passed == {"device": 0, "pin_memory": 0, "memory_format": 0, "non_contiguous": 0, "capture": 0, "other": 0}
