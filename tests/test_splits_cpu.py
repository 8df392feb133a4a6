"""CPU: the replica batch's host-side parts (sngnn_amd/splits.py) - the union edge list, the per-replica
early stopping, the reference's mean / std and what ``from_models`` refuses."""
import numpy as np
import pytest
import torch

import sngnn_amd
from sngnn_amd import splits as S


def test_union_edge_index_equals_a_per_replica_loop():
    gen = torch.Generator().manual_seed(3)
    n, e = 37, 120
    ei = torch.randint(0, n, (2, e), generator=gen)
    for r in (1, 2, 5):
        want = torch.cat([ei + k * n for k in range(r)], dim=1)
        got = S.union_edge_index(ei, n, r)
        assert torch.equal(got, want)
        assert got.is_contiguous() and got.dtype == ei.dtype


def test_union_size_is_refused_where_the_ids_would_overflow():
    S.check_union_size(7600, 30019, 50)
    with pytest.raises(ValueError, match="32-bit"):
        S.check_union_size(2 ** 20, 10, 2 ** 11)            # R N = 2^31
    with pytest.raises(ValueError, match="32-bit"):
        S.check_union_size(1000, 2 ** 28, 8)                # R (E + N) > 2^31
    with pytest.raises(ValueError):
        S.check_union_size(10, 10, 0)


def _reference_rule(seq, counts, patience):
    """train.train_graphed's loop (train.py:150-158) on one replica's recorded metrics."""
    final, bad, best, hist = 0.0, 0, float("inf"), []
    for epoch, m in enumerate(seq):
        rec = dict(val_loss=float(m[2]), test_acc=float(m[5]) / counts[2])
        hist.append(epoch)
        if rec["val_loss"] < best:
            best, final, bad = rec["val_loss"], rec["test_acc"], 0
        else:
            bad += 1
        if bad == patience:
            break
    return final, hist[-1], len(hist)


def test_early_stopping_per_replica_matches_the_trainers_rule():
    rng = np.random.default_rng(0)
    epochs, R, patience = 40, 6, 5
    seq = np.zeros((epochs, R, 6), dtype=np.float32)
    seq[:, :, [1, 3, 5]] = rng.integers(0, 100, (epochs, R, 3))
    seq[:, :, 0] = rng.random((epochs, R))
    # replica 0: falls then flat (ties never improve); 1: keeps improving; 2: noisy; 3: ties at the minimum;
    # 4: improves late after a long plateau shorter than the patience; 5: constant from the start
    seq[:, 0, 2] = np.maximum(1.0 - 0.1 * np.arange(epochs), 0.5)
    seq[:, 1, 2] = 2.0 - 0.01 * np.arange(epochs)
    seq[:, 2, 2] = rng.random(epochs)
    seq[:, 3, 2] = np.where(np.arange(epochs) < 3, 1.0 - 0.1 * np.arange(epochs), 0.7)
    seq[:, 4, 2] = np.concatenate([np.full(4, 1.0), np.full(4, 0.9), np.full(epochs - 8, 0.8)])
    seq[:, 5, 2] = 1.0
    counts = np.array([[40, 20, 30]] * R)
    es = S.EarlyStopping(R, patience, counts)
    for epoch in range(epochs):
        if es.update(epoch, seq[epoch]):
            break
    res = es.results()
    stops = set()
    for r in range(R):
        final, last, nhist = _reference_rule(seq[:, r], counts[r], patience)
        assert res[r]["final_test_acc"] == pytest.approx(final, abs=0), r
        assert res[r]["stop_epoch"] == last, r
        assert len(res[r]["history"]) == nhist, r
        assert [h["epoch"] for h in res[r]["history"]] == list(range(nhist))
        stops.add(last)
    assert len(stops) >= 3                     # the replicas stopped at different epochs
    assert res[1]["stopped"] is False and res[1]["stop_epoch"] == epochs - 1
    assert res[5]["stop_epoch"] == patience    # epoch 0 sets the best, epochs 1..5 are ties


def test_mean_std_is_the_reference_formula():
    accs = [0.3421, 0.3566, 0.3309, 0.3480, 0.3517, 0.3395, 0.3612, 0.3441, 0.3375, 0.3500]
    m, s = S.mean_std(accs)
    assert m == pytest.approx(np.mean(accs) * 100)
    assert s == pytest.approx(np.std(accs, ddof=1) * 100)
    assert "{:.2f}±{:.2f}".format(m, s) == "{:.2f}±{:.2f}".format(np.mean(accs) * 100, np.std(accs, ddof=1) * 100)


def test_repeat_for_betas_orders_split_major():
    tr = torch.tensor([[1, 0, 0], [0, 1, 0]], dtype=torch.bool)
    (m,), betas = S.repeat_for_betas([tr], [0.0, 0.5, 1.0])
    assert m.shape == (6, 3)
    assert torch.equal(m[0], tr[0]) and torch.equal(m[2], tr[0]) and torch.equal(m[3], tr[1])
    assert betas == [0.0, 0.5, 1.0, 0.0, 0.5, 1.0]


def _plus(f=12, c=5, n=30, k=1, thr=0.99, rem=0, layers=1, bn=False, beta=0.5, pp=False):
    torch.manual_seed(1234)
    if pp:
        return sngnn_amd.SNGNN_Plus_Plus(f, 16, c, n, layers, k, thr, beta, rem, 0.0, bn)
    return sngnn_amd.SNGNN_Plus(f, 16, c, n, layers, k, thr, rem, 0.0, bn)


def test_from_models_packs_and_unpacks_on_the_cpu():
    ms = [_plus(pp=True, beta=b) for b in (0.0, 0.3, 1.0)]
    with torch.no_grad():
        ms[1].lins[0].lin.weight.add_(1.0)
    batch = S.ReplicaBatch.from_models(ms)
    assert batch.R == 3 and tuple(batch.beta.tolist()) == pytest.approx((0.0, 0.3, 1.0))
    for r, m in enumerate(ms):
        got = batch.replica(r).state_dict()
        for k, v in m.state_dict().items():
            assert torch.equal(got[k], v), (r, k)


def test_from_models_rejects_what_it_cannot_batch():
    with pytest.raises(ValueError, match="top_k"):
        S.ReplicaBatch.from_models([_plus(k=1), _plus(k=2)])
    with pytest.raises(ValueError, match="thr"):
        S.ReplicaBatch.from_models([_plus(thr=0.99), _plus(thr=0.5)])
    with pytest.raises(ValueError, match="channels"):
        S.ReplicaBatch.from_models([_plus(c=5), _plus(c=6)])
    with pytest.raises(ValueError, match="channels"):
        S.ReplicaBatch.from_models([_plus(f=12), _plus(f=13)])
    with pytest.raises(ValueError, match="self-loop"):
        S.ReplicaBatch.from_models([_plus(rem=0), _plus(rem=1)])
    with pytest.raises(ValueError, match="num_layers"):
        S.ReplicaBatch.from_models([_plus(layers=2), _plus(layers=2)])
    with pytest.raises(ValueError, match="bn"):
        S.ReplicaBatch.from_models([_plus(bn=True)])
    with pytest.raises(ValueError, match="one class"):
        S.ReplicaBatch.from_models([_plus(), _plus(pp=True)])
    with pytest.raises(ValueError, match="AGNN"):
        S.ReplicaBatch.from_models([sngnn_amd.AGNN(12, 16, 5, 1)])
    with pytest.raises(ValueError):
        S.ReplicaBatch.from_models([])
