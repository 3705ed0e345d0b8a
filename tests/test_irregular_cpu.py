"""Batches of irregular packages without a GPU: data.collate_irregular, and what ERGB2DepthRecurrent.forward / the update primitives
refuse before any launch."""
import pytest
import torch


def _sample(n, Ce=5, H=8, W=12, depth=True):
    s = {"events": [torch.randn(Ce, H, W) for _ in range(n)], "image": torch.rand(1, H, W)}
    if depth:
        s["depth_events_last"] = torch.rand(1, H, W)
        s["depth_image_last"] = torch.rand(1, H, W)
    return s


def test_collate_irregular_pads_and_counts():
    from rpg_ramnet_amd.data import collate_irregular
    samples = [_sample(3), _sample(1), _sample(0), _sample(2)]
    item = collate_irregular(samples)
    assert [k for k in item if k.startswith("events")] == ["events0", "events1", "events2"]
    assert item["num_events"].tolist() == [3, 1, 0, 2] and item["num_events"].dtype == torch.int64
    assert item["image"].shape == (4, 1, 8, 12) and item["depth_image_last"].shape == (4, 1, 8, 12)
    for k in range(3):
        for b, s in enumerate(samples):
            if k < len(s["events"]):
                assert torch.equal(item["events%d" % k][b], s["events"][k])
            else:
                assert bool((item["events%d" % k][b] == 0).all())
    item = collate_irregular(samples, max_events=5)
    assert "events4" in item and "events5" not in item


def test_collate_irregular_errors():
    from rpg_ramnet_amd.data import collate_irregular
    with pytest.raises(ValueError):
        collate_irregular([])
    with pytest.raises(ValueError):
        collate_irregular([_sample(3)], max_events=2)
    with pytest.raises(ValueError):
        collate_irregular([_sample(2), _sample(1, H=6)])
    with pytest.raises(ValueError):
        collate_irregular([{"events": torch.randn(2, 5, 8, 12), "image": torch.rand(1, 8, 12)}])
    with pytest.raises(ValueError):
        collate_irregular([_sample(1), _sample(1, depth=False)])
    with pytest.raises(ValueError):
        collate_irregular([_sample(0), _sample(0)])


def _model(**over):
    from rpg_ramnet_amd.model.model import ERGB2DepthRecurrent
    cfg = dict(num_bins_rgb=1, num_bins_events=5, skip_type="sum", recurrent_block_type="conv", state_combination="convgru",
               num_encoders=2, base_num_channels=8, num_residual_blocks=1, use_upsample_conv=True, norm="none", gpu=0,
               every_x_rgb_frame=2, baseline=False, loss_composition=["image_last", "events_last"])
    cfg.update(over)
    return ERGB2DepthRecurrent(cfg)


def _item(counts, kmax=3):
    from rpg_ramnet_amd.data import collate_irregular
    item = collate_irregular([_sample(n) for n in counts], max_events=kmax)
    return item


@pytest.mark.parametrize("bad", [torch.tensor([1, 4]), torch.tensor([-1, 1]), torch.tensor([1.0, 2.0]), torch.tensor([1, 2, 3]),
                                 torch.tensor([True, False]), [1, 2]])
def test_forward_bad_num_events(bad):
    item = _item([1, 2])
    item["num_events"] = bad
    with pytest.raises(ValueError):
        _model()(item, None, None)


def test_forward_events_gap_and_shape():
    item = _item([1, 2])
    del item["events1"]
    with pytest.raises(ValueError):
        _model()(item, None, None)
    item = _item([1, 2])
    item["events1"] = item["events1"][:, :, :4]
    with pytest.raises(ValueError):
        _model()(item, None, None)


@pytest.mark.parametrize("over", [dict(baseline="e", state_combination="convlstm"), dict(recurrent_block_type="convlstm"),
                                  dict(norm="BN"), dict(norm="IN")])
def test_forward_irregular_refused_configurations(over):
    item = _item([1, 2])
    with pytest.raises(NotImplementedError):
        _model(**over)(item, None, None)


def test_update_primitives_refuse_masks_on_unsupported_configurations():
    m = _model(recurrent_block_type="convlstm")
    with pytest.raises(NotImplementedError):
        m.update_image(torch.rand(2, 1, 8, 12), None, active=torch.tensor([True, False]))


def test_active_mask_validation():
    from rpg_ramnet_amd import ops
    with pytest.raises(ValueError):
        ops.active_mask(torch.tensor([1.0, 0.0]), 2, torch.device("cpu"))
    with pytest.raises(ValueError):
        ops.active_mask(torch.tensor([1, 0, 1]), 2, torch.device("cpu"))
    assert ops.active_mask(torch.tensor([True, False]), 2, torch.device("cpu")).tolist() == [1, 0]
    assert ops.active_mask(None, 2, torch.device("cpu")) is None


def test_sequence_loss_dp_exact_refuses_irregular():
    from rpg_ramnet_amd.trainer import sequence_loss
    with pytest.raises(NotImplementedError):
        sequence_loss(_model(), [_item([1, 2])], ["image_last", "events_last"], [1, 1], dp_exact=True)
