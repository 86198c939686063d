"""Box-proposal recall without a GPU: `proposal_recall_metrics` on hand-made tables (the reference's float32 arithmetic, nan without
ground truth, keys and scaling, tables merge by addition), the default thresholds, the shape-only skip rule of the accumulator, and the
wrapper's rejections that need no device."""
import math

import pytest
import torch

KEYS = ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]


def _table(overlaps, thresholds):
    """(counts [T], num_pos) of one row from the recorded overlaps of its in-range ground truth"""
    ov = torch.tensor(overlaps, dtype=torch.float32)
    return (ov[:, None] >= thresholds[None, :]).sum(0), len(overlaps)


def test_default_thresholds_are_the_float32_arange():
    from ape_amd.evaluation import ProposalRecallAccumulator, proposal_recall_thresholds
    want = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    got = proposal_recall_thresholds()
    assert got.dtype == torch.float32 and got.numel() == 10 and torch.equal(got, want)
    acc = ProposalRecallAccumulator()
    assert acc.thresholds.dtype == torch.float32 and torch.equal(acc.thresholds, want)
    assert acc.names == KEYS


def test_metrics_keys_scaling_and_exact_recalls():
    from ape_amd.evaluation import proposal_recall_metrics
    # 4 ground-truth boxes; recalls 1, 1, .75, .75, .5, .5, .25, .25, 0, 0 are exact in float32 and so is their mean, 0.5
    row = [4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
    counts = torch.tensor([row, [4] * 10, [0] * 10, [2] * 10, row, row, [1] * 10, [3] * 10])
    num_pos = torch.tensor([4, 4, 4, 4, 4, 4, 4, 4])
    res = proposal_recall_metrics(counts, num_pos)
    assert list(res) == KEYS + ["gt"] and res["gt"] == 4
    assert [res[k] for k in KEYS] == [50.0, 100.0, 0.0, 50.0, 50.0, 50.0, 25.0, 75.0]
    assert all(type(res[k]) is float for k in KEYS)
    full = proposal_recall_metrics(counts, num_pos, images=7, thresholds=torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32))
    assert set(full) == set(KEYS) | {"images", "gt", "thresholds"} and full["images"] == 7
    assert full["thresholds"] == torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32).tolist()
    named = proposal_recall_metrics(counts[:2], num_pos[:2], names=["AR@10", "ARs@10"])
    assert named == {"AR@10": 50.0, "ARs@10": 100.0, "gt": 4}


def test_metrics_follow_the_reference_arithmetic():
    """recalls = float32 counts / Python float, mean in float32, x 100 on the Python float of the mean: thirds and sevenths do not come out
    as the float64 quotient would"""
    from ape_amd.evaluation import proposal_recall_metrics
    counts = torch.tensor([[3, 3, 2, 2, 2, 1, 1, 0, 0, 0], [7, 6, 5, 5, 4, 3, 2, 2, 1, 0]])
    num_pos = torch.tensor([3, 7])
    res = proposal_recall_metrics(counts, num_pos, names=["a", "b"])
    for c, k in enumerate(("a", "b")):
        recalls = torch.zeros(10, dtype=torch.float32)
        for t in range(10):
            recalls[t] = torch.tensor(float(counts[c, t]), dtype=torch.float32) / float(int(num_pos[c]))
        assert res[k] == float(recalls.mean().item() * 100)
    assert res["a"] != 100.0 * 14 / 30                          # the float64 quotient is another number


def test_metrics_without_ground_truth_are_nan():
    from ape_amd.evaluation import proposal_recall_metrics
    counts = torch.zeros((8, 10), dtype=torch.int64)
    counts[0] = 2
    num_pos = torch.tensor([2, 0, 2, 0, 2, 0, 2, 0])
    res = proposal_recall_metrics(counts, num_pos)
    assert res["AR@100"] == 100.0 and res["ARm@100"] == 0.0
    assert all(math.isnan(res[k]) for k in ("ARs@100", "ARl@100", "ARs@1000", "ARl@1000"))


def test_tables_merge_by_addition():
    from ape_amd.evaluation import proposal_recall_metrics, proposal_recall_thresholds
    thr = proposal_recall_thresholds()
    g = torch.Generator().manual_seed(5)
    streams = [[torch.rand(int(k), generator=g).tolist() for k in torch.randint(0, 9, (8,), generator=g)] for _ in range(2)]
    tables = []
    for rows in streams + [[a + b for a, b in zip(*streams)]]:
        parts = [_table(r, thr) for r in rows]
        tables.append((torch.stack([p[0] for p in parts]), torch.tensor([p[1] for p in parts])))
    (ca, na), (cb, nb), (cab, nab) = tables
    assert torch.equal(ca + cb, cab) and torch.equal(na + nb, nab)
    merged, whole = proposal_recall_metrics(ca + cb, na + nb), proposal_recall_metrics(cab, nab)
    assert all(merged[k] == whole[k] or (math.isnan(merged[k]) and math.isnan(whole[k])) for k in whole)


def test_metrics_reject_malformed_tables():
    from ape_amd.evaluation import proposal_recall_metrics
    with pytest.raises(ValueError):
        proposal_recall_metrics(torch.zeros((8, 10)), torch.zeros(8, dtype=torch.int64))          # float counts
    with pytest.raises(ValueError):
        proposal_recall_metrics(torch.zeros((8, 10), dtype=torch.int64), torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError):
        proposal_recall_metrics(torch.zeros((3, 10), dtype=torch.int64), torch.zeros(3, dtype=torch.int64))   # 3 rows, 8 default names
    with pytest.raises(ValueError):
        proposal_recall_metrics(torch.full((8, 10), 5), torch.full((8,), 4))                          # more hits than boxes


def test_images_without_proposals_or_ground_truth_add_nothing():
    """the skip rule looks at shapes alone and comes before any device work: it holds on a host without a GPU"""
    from ape_amd.evaluation import ProposalRecallAccumulator
    from ape_amd.structures import Boxes, Instances
    acc = ProposalRecallAccumulator(device="cpu")
    acc.update(None, torch.tensor([[0.0, 0.0, 10.0, 10.0]]), boxes=torch.zeros((0, 4)), logits=torch.zeros(0))
    acc.update(None, torch.zeros((0, 4)), boxes=torch.tensor([[0.0, 0.0, 10.0, 10.0]]), logits=torch.tensor([0.5]))
    acc.update(Instances((32, 32), proposal_boxes=Boxes(torch.zeros((0, 4))), objectness_logits=torch.zeros(0)), torch.rand(3, 4))
    acc.reduce()                                                # no process group: a no-op
    res = acc.compute()
    assert res["images"] == 3 and res["gt"] == 0 and int(acc.counts.sum()) == 0 and int(acc.num_pos.sum()) == 0
    assert all(math.isnan(res[k]) for k in KEYS)
    with pytest.raises(ValueError):
        acc.update(None, torch.rand(3, 4))                      # no proposals at all
    with pytest.raises(ValueError):
        acc.update(None, torch.rand(3, 4), boxes=torch.rand(5, 4), logits=torch.rand(4))
    with pytest.raises(TypeError):
        acc.update(torch.rand(5, 4), torch.rand(3, 4))          # bare tensors go in as boxes= / logits=
    with pytest.raises(RuntimeError):
        ProposalRecallAccumulator().compute()


def test_new_object_is_linked_behind_the_existing_ones():
    """the link order of the existing objects is what it was without boxcover.hip (alphabetical); the new object comes last (build.LINK_LAST
    says why)"""
    import os
    from ape_amd import build
    names = [os.path.basename(f) for f in build._sources()]
    assert names[-1] == "boxcover.hip" and names[:-1] == sorted(names[:-1]) and len(set(names)) == len(names)
    assert "-ffp-contract=off" in build.FILE_FLAGS["boxcover.hip"]


def test_wrapper_rejections_that_need_no_device():
    from ape_amd import ops
    p, g = torch.rand(5, 4), torch.rand(3, 4)
    with pytest.raises(RuntimeError):
        ops.box_cover_overlaps(p, g)                            # host tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        ops.box_cover_overlaps(p, g, gt_areas=torch.rand(3))
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p.double(), g)
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p, g.half())
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p, g, gt_areas=torch.rand(3).double())
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p[:, :3], g)                     # not [n, 4]
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g.reshape(-1))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(torch.rand(4, 5).t(), g)         # [5, 4] but not contiguous
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, gt_areas=torch.rand(4))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2)))                                      # a tensor on one side only
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2)), limits=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2)), limits=torch.zeros(2, dtype=torch.int64))
