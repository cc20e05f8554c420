"""The fp64 per-tap references of tests/exact_ref.py against PyTorch's own fp64 convolutions (CPU), and the measurement
that motivates the bit-exact GPU tests: a relative L2 check does not see one lost pixel."""

import pytest
import torch
import torch.nn.functional as F

from exact_ref import dgrad_ref, fwd_ref, ints, out_size, stem_form, ternary, ternary_density, wgrad_ref

# N, Ci, H, Co, k, s, p: ragged channels, odd images, strides that leave rows of the padded image unused
SHAPES = [
    (3, 72, 11, 200, 3, 2, 1),
    (2, 8, 9, 24, 3, 1, 1),
    (2, 16, 10, 8, 1, 2, 0),
    (2, 24, 7, 16, 1, 1, 0),
    (2, 4, 18, 16, 7, 2, 3),
    (1, 8, 8, 8, 3, 2, 1),
]


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_references_match_torch_fp64(shape):
    N, Ci, H, Co, k, s, p = shape
    OH = out_size(H, k, s, p)
    x = ints((N, H, H, Ci), -3, 3, 1)
    dy = ints((N, OH, OH, Co), -3, 3, 2)
    w = ints((Co, k, k, Ci), -3, 3, 3)
    wn = _nchw(w)
    assert torch.equal(wgrad_ref(dy, x, k, s, p),
                       torch.nn.grad.conv2d_weight(_nchw(x), (Co, Ci, k, k), _nchw(dy), s, p).permute(0, 2, 3, 1))
    assert torch.equal(fwd_ref(x, w, s, p), F.conv2d(_nchw(x), wn, None, s, p).permute(0, 2, 3, 1))
    assert torch.equal(dgrad_ref(dy, w, (H, H), s, p),
                       torch.nn.grad.conv2d_input((N, Ci, H, H), wn, _nchw(dy), s, p).permute(0, 2, 3, 1))


def test_references_non_square_image():
    N, Ci, H, W, Co = 2, 8, 4, 9, 16
    x = ints((N, H, W, Ci), -3, 3, 4)
    dy = ints((N, H, W, Co), -3, 3, 5)
    assert torch.equal(wgrad_ref(dy, x, 3, 1, 1),
                       torch.nn.grad.conv2d_weight(_nchw(x), (Co, Ci, 3, 3), _nchw(dy), 1, 1).permute(0, 2, 3, 1))


def test_generators():
    a = ints((4, 5, 5, 8), -3, 3, 7)
    assert a.dtype == torch.bfloat16 and torch.equal(a, ints((4, 5, 5, 8), -3, 3, 7))
    assert a.min() == -3 and a.max() == 3 and torch.equal(a, a.round())
    t = ternary((64, 3, 3, 64), 0.25, 8)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.2 < (t != 0).float().mean().item() < 0.3
    s = stem_form(ints((2, 6, 6, 4), -3, 3, 9))
    assert not s[..., 3].any() and s[..., :3].any()
    # the densities the GPU tests derive: 6 sigma of y below 256, a channel's sum(y * y) over M pixels below 2^23
    for K, M in [(4608, 1), (1152, 69580), (147, 37632)]:
        d = ternary_density(K, M)
        assert d <= 0.5 and 36 * K * d * d <= 256 ** 2 and M * K * d * d <= 0.6 * 2 ** 23 + 1e-6


def test_relative_l2_misses_one_lost_pixel():
    """3x3 stride-2 weight gradient, N = 2048, Ci = Co = 256, H = 6 (M = 18,432 output pixels), integer operands in
    [-3, 3]: zeroing ONE dY pixel changes most of the 589,824 output elements, and the relative L2 error of that
    result still passes the suite's `< 1e-2`. (All sums are of integers, exact in fp64: the gradient without the
    pixel is the full one minus that pixel's own contribution, computed from its image alone.)"""
    N, Ci, H, Co, k, s, p = 2048, 256, 6, 256, 3, 2, 1
    OH = out_size(H, k, s, p)
    x = ints((N, H, H, Ci), -3, 3, 0)
    dy = ints((N, OH, OH, Co), -3, 3, 1)
    ref = wgrad_ref(dy, x, k, s, p)
    n, oh, ow = 1000, 1, 1
    only = torch.zeros_like(dy[n:n + 1])
    only[0, oh, ow] = dy[n, oh, ow]
    lost = ref - wgrad_ref(only, x[n:n + 1], k, s, p)
    differ = (lost != ref).sum().item()
    rel = ((lost - ref).norm() / ref.norm()).item()
    print(f"one dY pixel of {N * OH * OH} zeroed: {differ} of {ref.numel()} elements differ, relative L2 {rel:.4f}")
    assert differ > 100_000
    assert rel < 1e-2
