"""Guarded scratch: every workspace the Python layer hands to the library becomes a slice of a larger uint8 tensor laid
out as ``[guard | payload | guard]``.

* payload: EXACTLY the bytes the library's size function returned (production pads to ``max(nbytes, 256)``), its base
  aligned to 256 bytes, filled with a poison pattern the caller chooses.  A returned 0 is an empty payload whose
  address is still the valid, non-NULL one between the two guards.
* guards: ``GUARD`` bytes each of the canary byte.  A kernel that writes past what its size function promised lands in
  them - valid memory of the harness's own - and :meth:`GuardedScratch.verify` finds it.

It patches, through pytest's ``monkeypatch`` (so the patches end with the test or the ``monkeypatch.context()``), the
three allocation points of the package: ``sngnn_amd.graph.Graph.scratch``, ``sngnn_amd._lib.workspace`` and
``sngnn_amd.ops._workspace`` (bound at import to the second).  The same key gives the same buffer inside one harness,
as in production: a graph's ``(entry, a, b, stream)``, a purpose's ``(key, device, stream)``.  One deliberate
difference: production keeps ONE grow-only buffer per purpose, so a smaller request gets the larger buffer; an exact
payload at every size and one buffer per purpose cannot both hold, and the exact payload is what finds an overrun, so
here a purpose asked for at another byte count gets a buffer of its own (the byte count is part of its key).  Contents
are only ever changed by :meth:`repoison`, so a stamp the library validates itself (the in-launch finalize's done
words) lives on between two calls as it does in use.

``records`` has one entry per buffer (what :meth:`damage` walks); ``handouts`` one per hand-out, repeats included.

A plain module, not a conftest: a test imports it and says when it is active.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

GUARD = 4096
ALIGN = 256
CANARY = 0xA5
POISON_NAN = 0x7FC12345          # as a word: a quiet NaN with a payload no kernel produces
POISON_ONES = b"\xff"            # a negative NaN, -1 in an integer region, all ones in a bitmap


class _Handout(torch.Tensor):
    """The payload slice.  ``data_ptr()`` is the payload's address even when it is empty (a plain empty tensor
    answers 0, and the library must see the non-NULL address between the guards)."""

    def data_ptr(self):
        return self._guarded_addr


class Record(NamedTuple):
    label: str               # the size entry (graph scratch) or the purpose (library workspace)
    args: tuple
    stream: Optional[int]
    nbytes: int
    base: torch.Tensor       # the whole [guard | pad | payload | guard | pad] tensor
    offset: int              # of the payload inside ``base``
    handout: torch.Tensor


def _pattern_bytes(pattern) -> bytes:
    if isinstance(pattern, int):
        return int(pattern).to_bytes(4, "little")
    pattern = bytes(pattern)
    if not pattern:
        raise ValueError("empty poison pattern")
    return pattern


def _fill(view: torch.Tensor, pattern) -> None:
    n = view.numel()
    if n == 0:
        return
    pat = torch.tensor(list(_pattern_bytes(pattern)), dtype=torch.uint8)
    view.copy_(pat.repeat(-(-n // pat.numel()))[:n].to(view.device))


class Handout(NamedTuple):
    label: str
    args: tuple
    stream: Optional[int]
    nbytes: int


class GuardDamage(AssertionError):
    pass


class GuardedScratch:
    def __init__(self, poison=POISON_NAN):
        self.poison = poison
        self.records: List[Record] = []          # one per buffer
        self.handouts: List[Handout] = []        # one per hand-out: entry or purpose, arguments, stream, bytes
        self._by_key = {}
        self._held = []          # objects whose id() is part of a key

    # ------------------------------------------------------------------ allocation
    def hand_out(self, label: str, args: tuple, stream, nbytes: int, device) -> torch.Tensor:
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError(f"{label}{args}: the size function returned {nbytes}")
        base = torch.empty(GUARD + ALIGN + nbytes + GUARD, dtype=torch.uint8, device=device)
        base.fill_(CANARY)
        offset = GUARD + (-(base.data_ptr() + GUARD)) % ALIGN
        _fill(base[offset:offset + nbytes], self.poison)
        handout = base[offset:offset + nbytes].as_subclass(_Handout)
        handout._guarded_addr = base.data_ptr() + offset
        self.records.append(Record(label, tuple(args), stream, nbytes, base, offset, handout))
        return handout

    def _get(self, key, label, args, stream, nbytes, device):
        hit = self._by_key.get(key)
        if hit is None:
            hit = self._by_key[key] = self.hand_out(label, args, stream, nbytes, device)
        self.handouts.append(Handout(label, tuple(args), stream, hit.numel()))
        return hit

    # ------------------------------------------------------------------ the three patches
    def install(self, monkeypatch) -> "GuardedScratch":
        from sngnn_amd import _lib, ops
        from sngnn_amd.graph import Graph
        harness = self

        def stream_of(device):
            return _lib.stream(device) if torch.device(device).type == "cuda" else None

        def scratch(graph, entry, a=None, b=None):
            stream = stream_of(graph.device)
            key = ("graph", id(graph), entry, a, b, stream)
            nbytes = 0
            if key not in harness._by_key:
                harness._held.append(graph)
                nbytes = int(getattr(_lib.load(), entry)(graph.handle, *(p for p in (a, b) if p is not None)))
            return harness._get(key, entry, (a, b), stream, nbytes, graph.device)

        def workspace(key, nbytes, device):
            stream = stream_of(device)
            return harness._get(("lib", key, str(device), stream, int(nbytes)), str(key), (int(nbytes),), stream,
                                nbytes, device)

        monkeypatch.setattr(Graph, "scratch", scratch)
        monkeypatch.setattr(_lib, "workspace", workspace)
        monkeypatch.setattr(ops, "_workspace", workspace)
        return self

    # ------------------------------------------------------------------ checks
    def repoison(self, pattern=None) -> None:
        """Refill every payload handed out so far (guards are left as they are: ``verify`` still sees old damage)."""
        if pattern is not None:
            self.poison = pattern
        for r in self.records:
            _fill(r.base[r.offset:r.offset + r.nbytes], self.poison)

    def labels(self):
        return {r.label for r in self.records}

    def damage(self) -> List[str]:
        """One line per damaged guard: the entry, the side and the first and last damaged byte - for ``after`` counted
        from the payload's end (0 = the first byte past it), for ``before`` from its start (-1 = the byte in front)."""
        found = []
        for r in self.records:
            end = r.offset + r.nbytes
            for side, lo, hi, origin in (("before", r.offset - GUARD, r.offset, r.offset), ("after", end, end + GUARD, end)):
                bad = (r.base[lo:hi] != CANARY).nonzero().flatten()
                if bad.numel():
                    first, last = int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin
                    found.append(f"{r.label}{r.args} ({r.nbytes} bytes, stream {r.stream}): guard {side} the payload "
                                 f"damaged, {bad.numel()} bytes, first at offset {first}, last at offset {last}")
        return found

    def verify(self) -> None:
        found = self.damage()
        if found:
            raise GuardDamage("a workspace was written outside its promised size:\n  " + "\n  ".join(found))
