"""The active node-range partition (``sngnn_amd.dist.Partition``): a leaf module, so the operators that refuse to run
under one (``prop``, ``gat``) can ask without importing ``dist``, which imports them through ``ops``."""
from __future__ import annotations

_current = None


def set_partition(part) -> None:
    """Make the conv layers treat their inputs as the local shard of ``part``
    (``None`` switches back to single-GPU behaviour)."""
    global _current
    _current = part


def current_partition():
    return _current
