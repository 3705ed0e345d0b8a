"""GPU: ops.switches against the launch-descriptor cache — one 3x3 convolution launched from one call site under four switch states in a
row.  A descriptor cached under one state and served under the next would launch the previous kernel: the library names the kernel of
every launch."""
import pytest
import torch
import torch.nn.functional as F

from rpg_ramnet_amd import _hip as Hh
from util import assert_close, nchw, nhwc

pytestmark = pytest.mark.gpu
TOL = 2e-4   # the suite's bound (tests/test_hip_ops.py): exact-fp32 MFMA vs PyTorch CPU; summation order differs


def test_a_switch_change_never_serves_a_cached_descriptor():
    """64 -> 64 channels, B = 1, 8 x 12: the smallest shape at which F(2x2,3x3), F(2x4,3x3) and F(2x4,3x3) on split operands are all
    eligible (the map of test_winograd_xcd_groups).  Every output against float64 F.conv2d; nothing leaks out of the contexts."""
    from rpg_ramnet_amd import ops
    dev = torch.device("cuda:0")
    B, H, W, ch = 1, 8, 12, 64
    torch.manual_seed(21)
    w, b, x = torch.randn(ch, ch, 3, 3) * 0.1, torch.randn(ch) * 0.1, torch.randn(B, ch, H, W)
    cp = ops.ConvParam([torch.nn.Parameter(w.to(dev))], [torch.nn.Parameter(b.to(dev))])
    xg = nhwc(x).to(dev).contiguous()
    taps = ops.Taps.get("conv", 3, 1)
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1).numpy()
    before = ops.switch_values()

    def launch(kernel, what):
        y = torch.full((B, H, W, ch), float("nan"), device=dev)
        ops.conv_launch(xg, taps, cp.fwd(), y, ch, bias=cp.bias())
        got = Hh.lib().ramnet_last_kernel().decode()
        assert got.startswith(kernel), (what, got)
        assert_close(nchw(y).cpu().numpy(), ref, TOL, what)

    launch("conv_wino_r_kernel", "defaults")
    with ops.switches(winograd_2x4="force"):
        launch("conv_wino_r6_kernel<", "winograd_2x4=force")
    with ops.switches(winograd_2x4="force", split_operands=True):
        launch("conv_wino_r6s_kernel<", "winograd_2x4=force, split_operands")
    launch("conv_wino_r_kernel", "defaults again")
    assert ops.switch_values() == before
