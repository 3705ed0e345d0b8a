"""CPU (no GPU): anchors of tests/grad_loss_restatement.py and the per-row conditions that the rules of tests/test_hip_grad_loss_launch.py
rely on (profiles/grad_loss_augment_tests_notes.md §1)."""
import pytest
import torch

from oracle import loss_ref
import grad_loss_cases as gc
import grad_loss_restatement as gr
import reduction_restatement as rr

F64 = torch.float64


def _pair(B, H, W, seed, kind, nan_share=0.0):
    gen = torch.Generator().manual_seed(seed)
    if kind == "int":
        p, t = (torch.randint(-16, 17, (B, H, W), generator=gen).to(F64) for _ in range(2))
    else:
        p, t = ((torch.randn(B, H, W, generator=gen).to(F64) * 1024).round() / 1024 for _ in range(2))         # pred - target is an fp32 number
    if nan_share:
        t[torch.rand(B, H, W, generator=gen) < nan_share] = float("nan")
    return p, t


ANCHORS = [(1, 8, 8, 4), (2, 9, 11, 2), (1, 21, 27, 3), (3, 16, 40, 4), (1, 13, 8, 1), (2, 70, 131, 4)]


@pytest.mark.parametrize("nan_share", [0.0, 0.05])
@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("B,H,W,ns", ANCHORS)
def test_against_the_oracle(B, H, W, ns, kind, nan_share):
    """the loss and its autograd gradient of oracle.loss_ref.multi_scale_grad_loss: a single pair (B = 1 of it) and the whole batch"""
    p, t = _pair(B, H, W, 7, kind, nan_share)
    for sl in (slice(0, 1), slice(0, B)):
        pp, tt = p[sl], t[sl]
        n = pp.shape[0]
        x = pp[:, None].clone().requires_grad_(True)
        ref = loss_ref.multi_scale_grad_loss(x, tt[:, None], num_scales=ns)
        st, _ = gr.stats(pp, tt, ns)
        got = gr.loss_from_stats(st, n)
        if bool(torch.isnan(ref)):
            assert bool(torch.isnan(got)) and bool((st[:, 1] == 0).any())
            continue
        assert abs(float(got) - float(ref.detach())) <= 1e-13 * abs(float(ref.detach()))
        ref.backward()
        grad, agrad = gr.backward(pp, tt, ns, st[:, 1], n * 2.0)
        assert float((grad - x.grad[:, 0]).abs().max()) <= 1e-13 * float(agrad.max())
        assert bool((grad.abs() <= agrad * (1 + 1e-12)).all()) and bool((agrad[torch.isnan(tt)] == 0).all())


@pytest.mark.parametrize("nan_share", [0.0, 0.2])
@pytest.mark.parametrize("B,H,W,ns", ANCHORS[:5])
def test_against_the_per_pair_statement(B, H, W, ns, nan_share):
    """reduction_restatement.msg_forward / msg_backward state the same loss with the pooling in fp32: on integer data the two agree"""
    p, t = _pair(B, H, W, 11, "int", nan_share)
    rstats, rloss, rws = rr.msg_forward(p, t, ns)
    st, _ = gr.stats(p, t, ns)
    assert torch.equal(st.reshape(-1), rstats)
    got = gr.loss_from_stats(st, B)
    assert (bool(torch.isnan(got)) and bool(torch.isnan(rloss))) or abs(float(got) - float(rloss)) <= 1e-14 * abs(float(rloss))
    given = st[:, 1] + 5.0
    rgiven = rstats.clone()
    rgiven[1::2] += 5.0
    rgrad, ragrad, _ = rr.msg_backward(rws, rgiven, B, H, W, ns, 0.75)
    grad, agrad = gr.backward(p, t, ns, given, 0.75 * B * 2.0)
    assert float((grad - rgrad).abs().max()) <= 1e-14 * max(float(ragrad.max()), 1e-300)
    assert float((agrad - ragrad).abs().max()) <= 1e-14 * max(float(ragrad.max()), 1e-300)


@pytest.mark.parametrize("kind", ["int", "normal"])
def test_statistics_of_shards_add_up(kind):
    p, t = _pair(5, 21, 27, 13, kind, 0.1)
    whole, _ = gr.stats(p, t, 3)
    parts = gr.stats(p[:2], t[:2], 3)[0] + gr.stats(p[2:], t[2:], 3)[0]
    assert torch.equal(whole[:, 1], parts[:, 1])
    if kind == "int":
        assert torch.equal(whole, parts)
    else:
        assert float((whole[:, 0] - parts[:, 0]).abs().max()) <= 1e-13 * float(whole[:, 0].max())


def test_workspace_and_scale_rules():
    assert gr.workspace_bytes(3, 2, 65, 129) == 3 * 2 * 2 * 3 * 64 and gr.workspace_bytes(1, 1, 64, 64) == 64
    assert gr.scales_ok(8, 21, 4) and not gr.scales_ok(7, 8, 4) and not gr.scales_ok(8, 8, 0) and not gr.scales_ok(64, 64, 5)


# ------------------------------------------------------------------------------------------------ the rows
@pytest.mark.parametrize("name", gc.INT_ROWS)
def test_integer_rows_are_exact(name):
    """diff, every pooled map (multiples of 1/64) and every response (multiples of 1/512) are fp32 numbers, and the sums stay below 2^53 / 512"""
    G, B, H, W, ns, _, _ = gc.ROWS[name]
    assert gr.scales_ok(H, W, ns) and B * H * W < 2 ** 31
    preds, targets = gc.data(name)
    for p, t in zip(preds, targets):
        diff = p - t
        ok = ~torch.isnan(diff)
        assert torch.equal(diff[ok], diff[ok].round()) and float(diff[ok].abs().max()) <= 32
        for s, (g, valid, ga) in enumerate(gr.responses(p, t, ns)):
            P = torch.nan_to_num(gr.pool(gr.f32(diff), s), nan=0.0)
            assert torch.equal(P * 64, (P * 64).round()) and torch.equal(g * 512, (g * 512).round())
            assert torch.equal(g.float().to(F64), g) and float(ga.sum()) * 512 < 2 ** 53
    st, _ = gc.statement(name)
    assert bool(torch.isfinite(st).all())


def test_rows_reach_what_they_are_for():
    R = gc.ROWS
    tiles = lambda n: (-(-R[n][2] // 64)) * (-(-R[n][3] // 64))
    assert tiles("m70x131") == 6 and tiles("join2") * R["join2"][1] > 32 and R["g70"][0] > 64
    assert sorted(R[n][3] % 4 for n in ("m64x64", "m63x66_ns4", "m65x67_ns4", "m66x69")) == [0, 1, 2, 3] and R["m72x136"][3] % 4 == 0
    for n in ("m8x8", "m8x21"):                     # the coarsest level is 1 x n: every vertical tap is clamped
        assert R[n][2] >> (R[n][4] - 1) == 1
    st, _ = gc.statement("empty")
    assert bool((st[1, :, 1] == 0).any()) and bool((st[1, :, 1] > 0).any()) and bool((st[0, :, 1] > 0).all()) and bool((st[2, :, 1] > 0).all())
    assert all(torch.equal(a, b) for k in (0, 2) for a, b in zip(gc.data("empty")[0][k:k + 1] + gc.data("empty")[1][k:k + 1],
                                                                 gc.data("empty_without")[0][k:k + 1] + gc.data("empty_without")[1][k:k + 1]))
    assert len(gc.HALO_PLACES) == 3 + 4 * len(gc.HALO_DIST) == R["halo"][0]
    for g, t in enumerate(gc.data("halo")[1]):
        assert int(torch.isnan(t).sum()) == 1
    st, _ = gc.statement("sample")
    assert bool((st[:, :, 1] > 0).all())


def test_normal_row_exclusions():
    """the share of pixels whose gradient is not compared (a response within reach lies within its own fp32 bound of zero): at most 0.1 %"""
    G, B, H, W, ns, _, _ = gc.ROWS["normal"]
    (p,), (t,) = gc.data("normal")
    bad = gr.unsafe_pixels(p, t, ns)
    print("normal row: %d of %d pixels excluded" % (int(bad.sum()), bad.numel()))
    assert int(bad.sum()) <= 0.001 * bad.numel()
