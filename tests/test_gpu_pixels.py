"""The pixel kernels on the device against the restatement of tests/pixels_ref.py: raw entry points on sentinel-filled outputs,
bit for bit wherever the contract fixes the bits (coordinates, colours, levels, the integer sums, the gradient), and within the
fp64 summation bound for the one sum whose order it does not fix."""
import ctypes

import pytest
import torch

import pixels_ref as R
from shacira_amd import _lib

pytestmark = pytest.mark.gpu
SENT = 12345.0
PAD = 3                    # rows behind the n the call may write: they keep the sentinel


def dev():
    return torch.device("cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    """fp32 / fp64 values as integers, every NaN as one pattern: equality of these is equality to the bit."""
    t = t.detach().cpu()
    ints = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return torch.where(torch.isnan(t), torch.full_like(ints, -1), ints)


def raw_batch(image, idx, start, n, want_coords=True, want_rgb=True):
    H, W = image.shape[:2]
    coords = torch.full((n + PAD, 2), SENT, device=dev()) if want_coords else None
    rgb = torch.full((n + PAD, 3), SENT, device=dev()) if want_rgb else None
    width = 0 if idx is None else (32 if idx.dtype == torch.int32 else 64)
    rc = _lib.lib().shacira_pixel_batch(ptr(image), H, W, ptr(idx), width, start, n, ptr(coords), ptr(rgb), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for out in (coords, rgb):
        if out is not None:
            assert (out[n:] == SENT).all(), "rows beyond n were written"
    return (coords[:n] if want_coords else None), (rgb[:n] if want_rgb else None)


def raw_loss(pred, image, idx, start, n, out_image=None):
    H, W = image.shape[:2]
    L = _lib.lib()
    nbytes = int(L.shacira_pixel_loss_workspace_bytes(n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev())
    stats = torch.full((3 + PAD,), SENT, dtype=torch.float64, device=dev())
    width = 0 if idx is None else (32 if idx.dtype == torch.int32 else 64)
    rc = L.shacira_pixel_loss_forward(ptr(pred), pred.stride(0) if pred.dim() == 2 and pred.shape[0] > 1 else 3, ptr(image), H, W,
                                      ptr(idx), width, start, n, ptr(out_image), ptr(stats), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (stats[3:] == SENT).all()
    return stats[:3].cpu()


def raw_grad(pred, image, idx, start, n, g):
    H, W = image.shape[:2]
    grad = torch.full((n + PAD, 3), SENT, device=dev())
    gdev = torch.tensor([g], dtype=torch.float32, device=dev())
    width = 0 if idx is None else (32 if idx.dtype == torch.int32 else 64)
    rc = _lib.lib().shacira_pixel_loss_backward(ptr(pred), pred.stride(0) if pred.shape[0] > 1 else 3, ptr(image), H, W, ptr(idx),
                                                width, start, n, ptr(gdev), ptr(grad), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (grad[n:] == SENT).all()
    return grad[:n]


def indices_for(n, hw, seed, dtype, bad=True):
    """n random pixels with duplicates; -1 and hw at rows 1 and 3 when there is room for valid neighbours."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, hw, (n,), generator=g, dtype=torch.int64)
    if n >= 2:
        idx[n - 1] = idx[0]                                   # a certain duplicate
    if bad and n >= 5:
        idx[1], idx[3] = -1, hw
    return idx.to(dtype)


@pytest.fixture(scope="module", params=R.IMAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def image_pair(request):
    H, W = request.param
    host = R.make_image(H, W)
    return host, host.to(dev())


def test_batch_is_bit_identical_to_the_restatement(image_pair):
    host, image = image_pair
    H, W = host.shape[:2]
    for n in R.N_LIST:
        for dtype in (torch.int32, torch.int64):
            idx = indices_for(n, H * W, n, dtype)
            want_c, want_rgb = R.pixel_batch_ref(host, idx)
            got_c, got_rgb = raw_batch(image, idx.to(dev()), 0, n)
            assert torch.equal(bits(got_c), bits(want_c)) and torch.equal(bits(got_rgb), bits(want_rgb)), (n, dtype)
            if n >= 5:                                        # NaN rows for -1 and H W, their neighbours are pixels
                assert torch.isnan(got_c[[1, 3]]).all() and torch.isnan(got_rgb[[1, 3]]).all()
                assert not torch.isnan(got_c[[0, 2, 4]]).any() and not torch.isnan(got_rgb[[0, 2, 4]]).any()
            only_c, none = raw_batch(image, idx.to(dev()), 0, n, want_rgb=False)
            assert none is None and torch.equal(bits(only_c), bits(want_c))
            none, only_rgb = raw_batch(image, idx.to(dev()), 0, n, want_coords=False)
            assert none is None and torch.equal(bits(only_rgb), bits(want_rgb))
        if n <= H * W:                                        # the range form: at 0, mid-image, ending exactly at H W
            for start in sorted({0, (H * W - n) // 2, H * W - n}):
                want_c, want_rgb = R.pixel_batch_ref(host, None, start, n)
                got_c, got_rgb = raw_batch(image, None, start, n)
                assert torch.equal(bits(got_c), bits(want_c)) and torch.equal(bits(got_rgb), bits(want_rgb)), (n, start)
    again = raw_batch(image, None, 0, min(H * W, 257))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, raw_batch(image, None, 0, min(H * W, 257))))


def test_batch_above_the_grid_cap_and_on_a_side_stream():
    from shacira_amd import hip_ops
    host = R.make_image(37, 53)
    image = host.to(dev())
    n = R.N_ABOVE_CAP                                         # more rows than the capped grid has lanes: the loop turns twice
    idx = indices_for(n, 37 * 53, 1, torch.int32)
    want_c, want_rgb = R.pixel_batch_ref(host, idx)
    got_c, got_rgb = raw_batch(image, idx.to(dev()), 0, n)
    assert torch.equal(bits(got_c), bits(want_c)) and torch.equal(bits(got_rgb), bits(want_rgb))
    side = torch.cuda.Stream()
    idx = indices_for(1025, 37 * 53, 2, torch.int64).to(dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c1, r1 = hip_ops.pixel_batch(image, idx)
        c2, r2 = raw_batch(image, idx, 0, 1025)
    side.synchronize()
    want_c, want_rgb = R.pixel_batch_ref(host, idx)
    assert torch.equal(bits(c1), bits(want_c)) and torch.equal(bits(r1), bits(want_rgb))
    assert torch.equal(bits(c2), bits(want_c)) and torch.equal(bits(r2), bits(want_rgb))
    c3, r3 = hip_ops.pixel_batch(image, idx.reshape(-1, 1), want_rgb=False)     # the [n, 1] indices of an 'eval' batch
    assert r3 is None and torch.equal(bits(c3), bits(want_c))
    c4, r4 = hip_ops.pixel_batch(image, None, start=100, n=0)
    assert tuple(c4.shape) == (0, 2) and tuple(r4.shape) == (0, 3)
    with pytest.raises(RuntimeError, match="not inside"):
        hip_ops.pixel_batch(image, None, start=37 * 53 - 4, n=5)
    with pytest.raises(RuntimeError, match="uint8"):
        hip_ops.pixel_batch(image.float())


def test_offsets_beyond_2_to_31_bytes():
    """A 32768 x 21846 image is 2 147 549 184 bytes: the last two rows lie beyond byte 2^31 - 1 - 131 076."""
    H, W = 32768, 21846
    assert H * W * 3 > 2 ** 31
    image = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev())
    tail = R.make_image(2, W)
    image[H - 2:] = tail.to(dev())
    g = torch.Generator().manual_seed(9)
    n = 1025
    local = torch.randint(0, 2 * W, (n,), generator=g, dtype=torch.int64)
    local[0], local[1] = 2 * W - 1, 0
    p = local + (H - 2) * W
    y, x = p // W, p % W
    want_c = torch.stack([(y.float() / float(H) - 0.5) * 2.0, (x.float() / float(W) - 0.5) * 2.0], dim=-1)
    want_rgb = tail.reshape(-1, 3)[local].float() / 255.0
    pred = R.pred_for(n, tail, local)
    want = R.pixel_loss_ref(pred, tail, local)
    pd = pred.to(dev())
    for dtype in (torch.int32, torch.int64):
        idx = p.to(dtype).to(dev())
        got_c, got_rgb = raw_batch(image, idx, 0, n)
        assert torch.equal(bits(got_c), bits(want_c)) and torch.equal(bits(got_rgb), bits(want_rgb)), dtype
        st = raw_loss(pd, image, idx, 0, n).tolist()
        assert (int(st[1]), int(st[2])) == (want["lvl"], want["count"]) and abs(st[0] - want["sq"]) <= 2 * 3 * n * 2.0 ** -53 * want["sq"]
        assert torch.equal(bits(raw_grad(pd, image, idx, 0, n, 0.5)), bits(R.pixel_grad_ref(pred, tail, local, 0, 0.5)))
    start = H * W - 257                                       # the range form, ending exactly at H W
    got_c, got_rgb = raw_batch(image, None, start, 257)
    assert torch.equal(bits(got_rgb), bits(tail.reshape(-1, 3)[2 * W - 257:].float() / 255.0))
    p = torch.arange(start, H * W, dtype=torch.int64)
    y, x = p // W, p % W
    want_c = torch.stack([(y.float() / float(H) - 0.5) * 2.0, (x.float() / float(W) - 0.5) * 2.0], dim=-1)
    assert torch.equal(bits(got_c), bits(want_c))


def check_loss(host, image, pred, idx, start, n):
    """One forward call against the restatement; returns the stats."""
    want = R.pixel_loss_ref(pred[:n], host, idx, start)
    got = raw_loss(pred.to(dev()), image, None if idx is None else idx.to(dev()), start, n)
    st = got.tolist()
    print(f"n {n} sq {st[0]!r} want {want['sq']!r} rel {abs(st[0] - want['sq']) / max(want['sq'], 1e-300):.3e} lvl {st[1]} count {st[2]}")
    assert st[1] == float(want["lvl"]) and st[2] == float(want["count"]) and int(st[1]) == want["lvl"]
    if want["sq"] != want["sq"]:
        assert st[0] != st[0]                                 # a NaN prediction shows in the squared error
    elif want["sq"] == float("inf"):
        assert st[0] == float("inf")
    else:
        assert abs(st[0] - want["sq"]) <= 2 * 3 * n * 2.0 ** -53 * want["sq"]
    return got


def test_loss_forward_statistics(image_pair):
    host, image = image_pair
    H, W = host.shape[:2]
    for n in R.N_LIST:
        if n == 0:
            stats = torch.full((3,), SENT, dtype=torch.float64, device=dev())
            assert _lib.lib().shacira_pixel_loss_forward(None, 3, ptr(image), H, W, None, 0, 0, 0, None, ptr(stats), None, 0,
                                                         stream()) == 0
            torch.cuda.synchronize()
            assert (stats == SENT).all()                      # nothing enqueued
            continue
        for dtype in (torch.int32, torch.int64):
            idx = indices_for(n, H * W, 50 + n, dtype)        # duplicates and two indices out of range
            pred = R.pred_for(n, host, idx)
            first = check_loss(host, image, pred, idx, 0, n)
            again = raw_loss(pred.to(dev()), image, idx.to(dev()), 0, n)
            assert torch.equal(bits(first), bits(again))      # two calls, the same bits
            if n >= 8:
                check_loss(host, image, R.add_nonfinite(pred), idx, 0, n)
        wide = R.pred_for(n, host, idx, width=5)              # a row-strided view: stride 5, three columns read
        check_loss(host, image, wide, idx, 0, n)
        if n <= H * W:
            for start in sorted({0, H * W - n}):
                check_loss(host, image, R.pred_for(n, host, None, start), None, start, n)


def test_loss_out_image_levels(image_pair):
    host, image = image_pair
    H, W = host.shape[:2]
    for n in (k for k in R.N_LIST if 0 < k <= H * W):
        idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(n))[:n]          # unique
        pred = R.add_nonfinite(R.pred_for(n, host, idx)) if n >= 8 else R.pred_for(n, host, idx)
        before = R.make_image(H, W, seed=5)
        out = before.to(dev())
        want = R.pixel_loss_ref(pred, host, idx)
        with_image = raw_loss(pred.to(dev()), image, idx.to(torch.int32).to(dev()), 0, n, out)
        without = raw_loss(pred.to(dev()), image, idx.to(torch.int32).to(dev()), 0, n)
        assert torch.equal(bits(with_image), bits(without))   # the statistics do not depend on the image output
        expect = before.clone().reshape(-1, 3)
        expect[idx] = want["levels"]
        assert torch.equal(out.cpu().reshape(-1, 3), expect)  # written pixels hold the levels, every other byte is as it was
        finite = torch.isfinite(pred).all(dim=1)
        chain = (torch.clamp(pred, 0, 1) * 255).to(torch.uint8)
        assert torch.equal(out.cpu().reshape(-1, 3)[idx][finite], chain[finite])              # the torch chain itself
        out2 = before.to(dev())                               # the range form writes the same places
        raw_loss(pred.to(dev()), image, None, H * W - n, n, out2)
        expect = before.clone().reshape(-1, 3)
        expect[H * W - n:] = R.pixel_loss_ref(pred, host, None, H * W - n)["levels"]
        assert torch.equal(out2.cpu().reshape(-1, 3), expect)


def test_gradient_is_bit_identical_to_autograd(image_pair):
    from shacira_amd import hip_ops
    host, image = image_pair
    H, W = host.shape[:2]
    for n in (k for k in R.N_LIST if k > 0):
        for dtype in (torch.int32, torch.int64):
            idx = indices_for(n, H * W, 90 + n, dtype, bad=False).to(dev())
            for width in (3, 5):
                base = R.pred_for(n, host, idx, width=width).to(dev())
                # the target as the host makes it (ToTensor): torch's DEVICE division by a scalar multiplies by a reciprocal
                gt = R.to_tensor_division(host)[idx.cpu().long()].to(dev())
                for k in (1.0, 1.0 / (3 * n)):
                    a = base.clone().requires_grad_(True)
                    (((a[:, :3] - gt) ** 2).sum() * k).backward()
                    b = base.clone().requires_grad_(True)
                    sq, stats = hip_ops.pixel_loss(b[:, :3], image, idx)
                    assert sq.dtype == torch.float32 and sq.dim() == 0 and not stats.requires_grad and stats.dtype == torch.float64
                    (sq * k).backward()
                    assert torch.equal(bits(a.grad), bits(b.grad)), (n, dtype, width, k)
                    if width > 3:                             # the wide tensor itself: columns beyond the third get zero
                        c = base.clone().requires_grad_(True)
                        (hip_ops.pixel_loss(c, image, idx)[0] * k).backward()
                        assert torch.equal(bits(a.grad), bits(c.grad)), (n, dtype, width, k)
        # skipped rows get zero, their neighbours the restatement's bits; the raw call on sentinel-filled rows
        idx = indices_for(n, H * W, 120 + n, torch.int64)
        pred = R.pred_for(n, host, idx)
        got = raw_grad(pred.to(dev()), image, idx.to(dev()), 0, n, 0.25)
        assert torch.equal(bits(got), bits(R.pixel_grad_ref(pred, host, idx, 0, 0.25)))
        if n >= 5:
            assert (got[[1, 3]] == 0).all()
    a = torch.zeros((4, 3), device=dev(), requires_grad=True)
    sq, _ = hip_ops.pixel_loss(a, image, None, start=0) if H * W >= 4 else (None, None)
    if sq is not None:
        (g,) = torch.autograd.grad(sq, a, create_graph=True)
        with pytest.raises(RuntimeError):                     # once differentiable
            g.sum().backward()


def test_loss_and_gradient_above_the_grid_cap():
    host = R.make_image(37, 53)
    image = host.to(dev())
    n = R.N_ABOVE_CAP
    idx = indices_for(n, 37 * 53, 3, torch.int32)
    pred = R.pred_for(n, host, idx)
    first = check_loss(host, image, pred, idx, 0, n)
    assert torch.equal(bits(first), bits(raw_loss(pred.to(dev()), image, idx.to(dev()), 0, n)))
    got = raw_grad(pred.to(dev()), image, idx.to(dev()), 0, n, 1.0 / (3 * n))
    assert torch.equal(bits(got), bits(R.pixel_grad_ref(pred, host, idx, 0, 1.0 / (3 * n))))
