"""The guarded-scratch harness (tests/guarded_scratch.py) on CPU tensors: it reports one byte written on either side
of a payload at the right offset, passes an untouched run, hands out a non-NULL address for zero bytes, keeps one buffer
per key, and its three patches end with the monkeypatch context."""
import pytest
import torch

from tests import guarded_scratch as GS

CPU = torch.device("cpu")


def _harness(monkeypatch, poison=GS.POISON_NAN):
    return GS.GuardedScratch(poison).install(monkeypatch)


def test_an_untouched_run_passes_and_the_payload_is_exact_aligned_and_poisoned(monkeypatch):
    from sngnn_amd import _lib
    h = _harness(monkeypatch)
    ws = _lib.workspace("wgrad", 1000, CPU)
    assert ws.numel() == 1000 and ws.dtype == torch.uint8 and ws.is_contiguous()
    assert ws.data_ptr() % GS.ALIGN == 0
    rec = h.records[0]
    assert (rec.label, rec.args, rec.stream, rec.nbytes) == ("wgrad", (1000,), None, 1000)
    assert rec.base.data_ptr() + rec.offset == ws.data_ptr() and rec.offset >= GS.GUARD
    assert rec.base.numel() >= rec.offset + 1000 + GS.GUARD
    assert bytes(ws.tolist()[:8]) == (0x7FC12345).to_bytes(4, "little") * 2
    assert torch.frombuffer(bytearray(ws.tolist()), dtype=torch.float32).isnan().all()
    ws.fill_(0)                         # the whole payload may be written
    h.verify()
    assert h.damage() == []


@pytest.mark.parametrize("nbytes", [1000, 1, 0])
@pytest.mark.parametrize("side,where,offset", [("after", 0, 0), ("after", 300, 300), ("after", GS.GUARD - 1, GS.GUARD - 1),
                                               ("before", -1, -1), ("before", -GS.GUARD, -GS.GUARD)])
def test_one_byte_outside_the_payload_is_reported_at_its_offset(monkeypatch, nbytes, side, where, offset):
    from sngnn_amd import _lib
    h = _harness(monkeypatch)
    _lib.workspace("quiet", 64, CPU)
    _lib.workspace("bn_train", nbytes, CPU)
    rec = h.records[1]
    origin = rec.offset + (nbytes if side == "after" else 0)
    rec.base[origin + where] = 0
    lines = h.damage()
    assert len(lines) == 1, lines
    assert "bn_train" in lines[0] and f"guard {side} the payload" in lines[0]
    assert f"first at offset {offset}, last at offset {offset}" in lines[0] and "1 bytes" in lines[0]
    with pytest.raises(GS.GuardDamage, match="bn_train"):
        h.verify()


def test_a_run_of_damaged_bytes_reports_first_and_last(monkeypatch):
    from sngnn_amd import _lib
    h = _harness(monkeypatch)
    _lib.workspace("head", 512, CPU)
    rec = h.records[0]
    rec.base[rec.offset + 512 + 4: rec.offset + 512 + 260] = 1
    assert "256 bytes, first at offset 4, last at offset 259" in h.damage()[0]


def test_zero_bytes_is_an_empty_payload_at_a_valid_address(monkeypatch):
    from sngnn_amd import _lib
    h = _harness(monkeypatch)
    ws = _lib.workspace("blend", 0, CPU)
    rec = h.records[0]
    assert ws.numel() == 0 and rec.nbytes == 0
    assert ws.data_ptr() != 0 and ws.data_ptr() == rec.base.data_ptr() + rec.offset and ws.data_ptr() % GS.ALIGN == 0
    assert _lib.ptr(ws) == ws.data_ptr()
    assert bool((rec.base == GS.CANARY).all())          # nothing but guards around it
    h.verify()


def test_same_key_same_buffer_and_repoison(monkeypatch):
    from sngnn_amd import _lib, ops
    h = _harness(monkeypatch, GS.POISON_ONES)
    a = _lib.workspace("head", 300, CPU)
    assert _lib.workspace("head", 300, CPU) is a and ops._workspace("head", 300, CPU) is a
    assert len(h.records) == 1
    assert h.handouts == [GS.Handout("head", (300,), None, 300)] * 3          # every hand-out, repeats included
    b = _lib.workspace("head", 301, CPU)          # another size: an exact payload of its own
    assert b is not a and b.numel() == 301 and len(h.records) == 2
    assert _lib.workspace(("glognn_gram", 7), 300, CPU) is not a
    assert h.labels() == {"head", "('glognn_gram', 7)"}
    assert bool((a == 0xFF).all())
    a.fill_(3)
    h.repoison()
    assert bool((a == 0xFF).all())
    h.repoison(GS.POISON_NAN)
    assert bytes(b.tolist()[:5]) == b"\x45\x23\xc1\x7f\x45"
    h.verify()


def test_graph_scratch_is_sized_by_the_library_entry_and_keyed_like_production(monkeypatch):
    """``Graph.scratch`` through the harness, with a stand-in for the library and the graph (no GPU here)."""
    from sngnn_amd import _lib
    from sngnn_amd.graph import Graph

    class _Lib:
        @staticmethod
        def sngnn_graph_workspace_bytes(handle, c):
            return handle * c

        @staticmethod
        def sngnn_two_hop_workspace_bytes(handle):
            return 0

    class _G:
        device, handle = CPU, 10

    h = _harness(monkeypatch)
    monkeypatch.setattr(_lib, "load", lambda: _Lib)
    _G.scratch, _G.workspace = Graph.scratch, Graph.workspace          # (the patched scratch)
    g, g2 = _G(), _G()
    ws = g.workspace(5)
    assert ws.numel() == 50 and g.workspace(5) is ws and g.workspace(6) is not ws and g2.workspace(5) is not ws
    z = g.scratch("sngnn_two_hop_workspace_bytes")
    assert z.numel() == 0 and z.data_ptr() != 0
    assert [(r.label, r.args, r.nbytes) for r in h.records] == [
        ("sngnn_graph_workspace_bytes", (5, None), 50), ("sngnn_graph_workspace_bytes", (6, None), 60),
        ("sngnn_graph_workspace_bytes", (5, None), 50), ("sngnn_two_hop_workspace_bytes", (None, None), 0)]
    assert [(r.label, r.args, r.nbytes) for r in h.handouts] == [
        ("sngnn_graph_workspace_bytes", (5, None), 50), ("sngnn_graph_workspace_bytes", (5, None), 50),
        ("sngnn_graph_workspace_bytes", (6, None), 60), ("sngnn_graph_workspace_bytes", (5, None), 50),
        ("sngnn_two_hop_workspace_bytes", (None, None), 0)]
    h.verify()


def test_the_three_patches_are_undone_on_exit(monkeypatch):
    from sngnn_amd import _lib, ops
    from sngnn_amd.graph import Graph
    before = (Graph.__dict__["scratch"], _lib.workspace, ops._workspace)
    assert before[1] is before[2]
    with monkeypatch.context() as m:
        GS.GuardedScratch().install(m)
        inside = (Graph.__dict__["scratch"], _lib.workspace, ops._workspace)
        assert all(a is not b for a, b in zip(before, inside)) and inside[1] is inside[2]
    assert (Graph.__dict__["scratch"], _lib.workspace, ops._workspace) == before
