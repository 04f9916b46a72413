"""Host logic of the batch training path (no GPU): grouping of scenes into batches, collation, GT offsets, per-segment
sampling and the argument checks of box_ops.match_segments."""
import pytest
import torch


def test_group_batches():
    from detection_3d_amd.engine import group_batches
    assert list(group_batches(range(5), 2)) == [[0, 1], [2, 3], [4]]
    assert list(group_batches(range(4), 1)) == [[0], [1], [2], [3]]
    assert list(group_batches([], 3)) == []
    with pytest.raises(ValueError):
        list(group_batches(range(3), 0))


def test_collate_appends_the_example_index():
    from detection_3d_amd.engine import collate

    def vox(pcl, cfg):                   # stand-in for d3d_voxelize: one voxel per point, shifted by the scene's minimum
        c = pcl[:, :3].long()
        return c - c.min(0)[0], pcl[:, 3:]

    scenes = [(torch.tensor([[3., 4., 5., 1.], [4., 4., 6., 2.]]), {"labels": torch.tensor([1])}),
              (torch.tensor([[7., 1., 0., 3.]]), {"labels": torch.tensor([2, 3])})]
    points, tgs = collate(scenes, None, vox)
    coords, feats, B = points
    assert B == 2 and coords.shape == (3, 4) and feats.shape == (3, 1)
    assert coords[:, 3].tolist() == [0, 0, 1]
    assert coords[:2, :3].tolist() == [[0, 0, 0], [1, 0, 1]] and coords[2, :3].tolist() == [0, 0, 0]
    assert [t["labels"].tolist() for t in tgs] == [[1], [2, 3]]
    with pytest.raises(ValueError):
        collate([], None, vox)


def test_segment_offsets():
    from detection_3d_amd.training import segment_offsets
    gt, offs = segment_offsets([torch.ones(2, 7), torch.zeros(0, 7), 2 * torch.ones(3, 7)])
    assert offs == [0, 2, 2, 5] and gt.shape == (5, 7) and gt[4, 0] == 2
    assert segment_offsets([]) == (None, [0])


def test_sample_segments_per_segment_budget():
    from detection_3d_amd.training import sample_segments

    class First(object):
        def __call__(self, labels):
            pos = torch.nonzero(labels >= 1).squeeze(1)[:2]
            neg = torch.nonzero(labels == 0).squeeze(1)[:3]
            return pos, neg

    labels = torch.tensor([1., 0., 1., 0., 1., 0., 1., -1., 0., 0.])
    seg = torch.tensor([0, 1, 0, 1, 1, 0, 0, 1, 1, 2])
    pos, neg = sample_segments(First(), labels, seg, 4)
    assert [p.tolist() for p in pos] == [[0, 2], [4], [], []]
    assert [n.tolist() for n in neg] == [[5], [1, 3, 8], [9], []]


def test_match_segments_argument_checks():
    from detection_3d_amd import _lib, box_ops
    gt, pred = torch.zeros(3, 7), torch.zeros(4, 7)
    seg = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.D3DError):                        # no CPU fallback
        box_ops.match_segments(gt, [0, 3], pred, seg)
    with pytest.raises(ValueError):
        box_ops.match_segments(gt, [1, 3], pred, seg)          # offsets must start at 0
    with pytest.raises(ValueError):
        box_ops.match_segments(gt, [0, 2, 1], pred, seg)       # and not decrease
    with pytest.raises(ValueError):
        box_ops.match_segments(gt, [0] * 300, pred, seg)       # at most 256 segments
    with pytest.raises(ValueError):
        box_ops.match_segments(gt, [], pred, seg)


def test_match_segments_scratch_bytes():
    from detection_3d_amd._lib import lib
    n = lib().d3d_match_segments_scratch_bytes(1000, 500000)
    assert n >= 2 * 4 * 500000 + 4 * 1000
    assert lib().d3d_match_segments_scratch_bytes(0, 0) > 0
