"""The guard-band helper (tests/guards.py) must itself fail when it should: CPU tensors, a stand-in "op" module whose ``torch`` is proxied."""
import pytest
import torch

from tests import guards

@pytest.fixture()
def standin():
    return guards.standin_module()


def bits(t):
    return guards.raw(t)


def test_correct_op_passes_and_is_bit_identical_under_both_poisons(standin):
    x = torch.randn(5, 37).half()
    outs = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(standin):
            assert standin.torch is g.proxy
            y = standin.scale_rows(g.guard_input(x))
        assert standin.torch is torch                      # restored; the global torch was never touched
        g.check()
        assert len(g.records) == 2 and [r.what for r in g.records] == ["input", "empty"]
        outs.append(y)
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(outs[0], x * 2)


def test_monkeypatch_route_installs_the_same_proxy(standin, monkeypatch):
    g = guards.Guard(0x5A)
    monkeypatch.setattr(standin, "torch", g.proxy)
    y = standin.scale_rows(torch.ones(3, 4))
    g.check()
    assert g.records[0].shape == (3, 4) and torch.equal(y, torch.full((3, 4), 2.0))
    assert standin.torch.float16 is torch.float16 and standin.torch.Tensor is torch.Tensor     # everything else is forwarded


@pytest.mark.parametrize("poison", guards.POISONS)
def test_one_byte_past_the_payload_fails_with_back_and_names_the_offset(standin, poison):
    g = guards.Guard(poison)
    with g.on(standin):
        y = standin.sized(74)
    rec = g.records[0]
    rec.buf[rec.front + 74] = 0x11                         # the byte right behind the payload: no rounding up to 16
    with pytest.raises(guards.GuardError) as e:
        g.check()
    msg = str(e.value)
    assert "back pad" in msg and "front pad" not in msg
    assert "first at payload offset 74, last at 74" in msg and "shape=(74,)" in msg and "torch.uint8" in msg
    assert y.numel() == 74


@pytest.mark.parametrize("poison", guards.POISONS)
def test_one_byte_before_the_payload_fails_with_front_and_names_the_offset(standin, poison):
    g = guards.Guard(poison)
    with g.on(standin):
        standin.scale_rows(torch.zeros(3, 9, dtype=torch.float16))
    rec = g.records[0]
    rec.buf[rec.front - 1] = 0x11
    rec.buf[rec.front - 40] = 0x11
    with pytest.raises(guards.GuardError) as e:
        g.check()
    msg = str(e.value)
    assert "front pad" in msg and "back pad" not in msg
    assert "first at payload offset -40, last at -1" in msg and "shape=(3, 9)" in msg and "torch.float16" in msg


def test_unwritten_last_row_gives_different_bits_under_the_two_poisons(standin):
    x = torch.randn(4, 16).half()
    outs = []
    for poison in guards.POISONS:
        g = guards.Guard(poison)
        with g.on(standin):
            outs.append(standin.skips_last_row(x))
        g.check()                                          # nothing out of bounds: only the two-poison comparison can see this
    assert torch.equal(bits(outs[0][:-1]), bits(outs[1][:-1]))
    assert not torch.equal(bits(outs[0]), bits(outs[1]))
    assert not guards.same_raw(outs[0], outs[1])
    assert bool((bits(outs[0][-1]) == 0x5A).all()) and bool((bits(outs[1][-1]) == 0xA5).all())


@pytest.mark.parametrize("poison", guards.POISONS)
def test_zeros_payload_is_zero_and_its_pads_are_poison(standin, poison):
    g = guards.Guard(poison)
    with g.on(standin):
        c = standin.counters(33)
        f = standin.filled(7)
        b = standin.flags(9)
    assert c.dtype == torch.int32 and c.shape == (33,) and not c.any() and not b.any()
    assert f.dtype == torch.float16 and bool((f == 3).all())
    for rec in g.records:
        for _, pad, _ in rec.pads():
            # an int32 tensor made with zeros is an index tensor: its pads hold a valid entry (zeros); every other pad is poison
            assert pad.numel() >= guards.PAD_FLOOR and bool((pad == (0 if rec.dtype == torch.int32 else poison)).all())
    g.check()
    g.records[0].buf[g.records[0].front + 33 * 4 + 2] = 7              # a stray store behind the index tensor is still seen
    with pytest.raises(guards.GuardError, match="back pad of zeros tensor"):
        g.check()
    g.records[0].buf[g.records[0].front + 33 * 4 + 2] = 0
    assert g.payload_bytes(c).numel() == 33 * 4 and g.find("zeros", 33 * 4)[0] is g.records[0]


@pytest.mark.parametrize("nbytes", [2, 9, 74, 9472])
def test_views_are_aligned_and_contiguous(standin, nbytes):
    g = guards.Guard(0xA5)
    with g.on(standin):
        v = standin.sized(nbytes)
        rows = g.proxy.empty((3, nbytes), dtype=torch.uint8)
    for t in (v, rows, g.guard_input(torch.zeros(5, nbytes, dtype=torch.uint8))):
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    rec = g.records[0]
    assert rec.front % 256 == 0 and rec.buf.numel() == 2 * rec.front + nbytes       # the back pad starts at the payload's last byte + 1
    assert bool((v == 0xA5).all())
    g.check()


def test_pad_sizes_follow_the_tile_rule():
    assert guards.pad_bytes((16, 4096), 2) == 2 << 20 == guards.PAD_CAP            # 256 rows of 8 KiB
    assert guards.pad_bytes((700, 74), 1) == guards.PAD_FLOOR                      # 256 rows of 74 bytes: the floor
    assert guards.pad_bytes((300, 512), 2) == 256 * 1024                           # 256 further rows of the tensor's own row size
    assert guards.pad_bytes((16384, 8192), 2) == guards.PAD_CAP
    assert all(guards.pad_bytes(s, 2) % 256 == 0 for s in [(1,), (3, 37), (2, 9, 5), ()])


def test_index_inputs_get_valid_entries_and_integer_tensors_refuse_nan():
    g = guards.Guard(0x5A)
    indptr = torch.tensor([0, 3, 7, 12], dtype=torch.int32)
    v = g.guard_input(indptr)                                                       # auto: a repeat of the last valid entry
    rec = g.records[-1]
    assert torch.equal(v, indptr)
    for _, pad, _ in rec.pads():
        assert bool((pad.view(torch.int32) == 12).all())
    z = g.guard_input(torch.tensor([5, 6], dtype=torch.int64), pad="zeros")
    assert torch.equal(z, torch.tensor([5, 6])) and not g.records[-1].buf[:g.records[-1].front].any()
    g.guard_input(torch.zeros(0, dtype=torch.int32))                                # nothing to repeat: zeros
    assert not g.records[-1].buf.any()
    for pad in ("nan", "ff"):
        with pytest.raises(TypeError):
            g.guard_input(indptr, pad=pad)
    with pytest.raises(TypeError):
        g.guard_input(torch.zeros(4, dtype=torch.uint8), pad="nan")
    g.check()


def test_float_and_byte_inputs_get_pads_that_would_change_a_result():
    x = torch.randn(3, 8)
    for poison, byte in zip(guards.POISONS, (0xFF, 0x88)):
        g = guards.Guard(poison)
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            v = g.guard_input(x.to(dt))
            rec = g.records[-1]
            assert torch.equal(v, x.to(dt))
            for _, pad, _ in rec.pads():
                assert bool(pad.view(dt).isnan().all())
        if poison == 0x5A:
            assert bool((g.records[0].buf[:16] == 0x7E).all())                      # fp16: 0x7E7E...
        q = g.guard_input(torch.arange(18, dtype=torch.uint8).reshape(2, 9))
        assert bool((g.records[-1].buf[:g.records[-1].front] == byte).all()) and q[1, 8] == 17
        g.check()


def test_a_damaged_input_pad_is_reported_too():
    g = guards.Guard(0xA5)
    g.guard_input(torch.ones(4, dtype=torch.float16))
    rec = g.records[0]
    rec.buf[rec.front + rec.nbytes + 5] = 0
    with pytest.raises(guards.GuardError, match="back pad of input tensor"):
        g.check()


def test_the_proxy_refuses_what_it_does_not_implement(standin):
    g = guards.Guard(0x5A)
    with g.on(standin):
        with pytest.raises(TypeError, match="pin_memory"):
            standin.pinned(4)
        with pytest.raises(TypeError, match="contiguous"):
            standin.scale_rows(torch.zeros(4, 6).t())
        with pytest.raises(TypeError, match="memory_format"):
            g.proxy.empty_like(torch.zeros(2, 2), memory_format=torch.contiguous_format)
        assert g.proxy.zeros((2, 1), requires_grad=False).shape == (2, 1)          # (deploy.nn.Linear4bit's buffers ask for exactly this)
        with pytest.raises(TypeError, match="requires_grad"):
            g.proxy.zeros((2, 1), requires_grad=True)
