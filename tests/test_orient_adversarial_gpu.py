"""orient_rbrief_kernel through the C ABI on the adversarial cases of tests/orb_ref.py, against its plain statement
(itself pinned against the C oracle, and against answers that follow from the tables alone, by tests/test_orb_ref.py):
exact bin ties inside and across the kernel's lane groups, saturated moments, single-pixel descriptor planes, planes
full of equal values, every pixel of small images as a keypoint (both sides of the patch loaders' fast path at every
byte alignment; pitches wider than the image, odd, and off dword boundaries), image counts around the 8-way block map
and keypoint counts around max_kp.  Every case runs through every entry point that accepts it; angles and descriptors
bit for bit; every output slot is pre-filled and must be written, a guard row either side must not be; the inputs
must come back unchanged."""
import numpy as np
import pytest
import torch

import orb_ref as R
from visual_underwater_slam_amd.frontend import tile_planes

pytestmark = pytest.mark.gpu

DESC_FILL, ANG_FILL, ORDER_FILL = 0x5A5A5A5A5A5A5A5A, 99, -7


def _L():
    import visual_underwater_slam_amd._lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the cases are shared and read-only


def _guarded(n, row, fill, dtype):
    """A [n, row] view with one guard row either side inside one pre-filled buffer: (buffer, view)."""
    buf = torch.full(((n + 2) * row,), fill, dtype=dtype, device="cuda")
    return buf, buf[row:(n + 1) * row]


def gpu_order(keys_d, counts_d, n, max_kp, H, W):
    """vus_orient_order into a guarded, pre-filled buffer: the order [n, max_kp] as numpy and on the device."""
    L = _L()
    buf, order = _guarded(n, max_kp, ORDER_FILL, torch.int32)
    L.call("vus_orient_order", keys_d.data_ptr(), counts_d.data_ptr(), n, max_kp, H, W, order.data_ptr(), L.current_stream_ptr())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:max_kp] == ORDER_FILL).all() and (b[-max_kp:] == ORDER_FILL).all(), "vus_orient_order wrote outside its rows"
    return b[max_kp:-max_kp].reshape(n, max_kp), order


def shuffled_order(counts, max_kp, seed):
    rng = np.random.default_rng(seed)
    perm = np.tile(np.arange(max_kp, dtype=np.int32), (len(counts), 1))
    for i, c in enumerate(counts):
        c = R.live_count(c, max_kp)
        perm[i, :c] = rng.permutation(c)
    return perm


def run_entry(entry, img_d, blur_d, keys_d, counts_d, order_d, n, H, W, pitch, max_kp):
    """One launch with guarded, pre-filled outputs: (desc u64 [n, max_kp, 4], angle u8 [n, max_kp]) as numpy."""
    L = _L()
    dbuf, desc = _guarded(n, max_kp * 4, DESC_FILL, torch.int64)
    abuf, ang = _guarded(n, max_kp, ANG_FILL, torch.uint8)
    st = L.current_stream_ptr()
    if entry == "plain":
        L.call("vus_orient_rbrief", img_d.data_ptr(), blur_d.data_ptr(), n, H, W, pitch, keys_d.data_ptr(), counts_d.data_ptr(),
               max_kp, desc.data_ptr(), ang.data_ptr(), st)
    elif entry == "ordered":
        L.call("vus_orient_rbrief_ordered", img_d.data_ptr(), blur_d.data_ptr(), n, H, W, pitch, keys_d.data_ptr(),
               counts_d.data_ptr(), max_kp, order_d.data_ptr(), desc.data_ptr(), ang.data_ptr(), st)
    else:
        assert entry == "tiled"
        L.call("vus_orient_rbrief_tiled", img_d.data_ptr(), blur_d.data_ptr(), n, H, W, keys_d.data_ptr(), counts_d.data_ptr(),
               max_kp, L.ptr(order_d), desc.data_ptr(), ang.data_ptr(), st)
    torch.cuda.synchronize()
    d, a = dbuf.cpu().numpy().view(np.uint64), abuf.cpu().numpy()
    g = max_kp * 4
    assert (d[:g] == DESC_FILL).all() and (d[-g:] == DESC_FILL).all(), f"{entry}: descriptors written outside their rows"
    assert (a[:max_kp] == ANG_FILL).all() and (a[-max_kp:] == ANG_FILL).all(), f"{entry}: angles written outside their rows"
    return d[g:-g].reshape(n, max_kp, 4), a[max_kp:-max_kp].reshape(n, max_kp)


def check_case(name, entries=None):
    img, blur, keys, counts, meta, ref = R.image_case(name)
    H, W, pitch = meta["H"], meta["W"], meta["pitch"]
    n, max_kp = keys.shape
    img_d, blur_d, keys_d, counts_d = _dev(img), _dev(blur), _dev(keys.view(np.int32)), _dev(counts)
    cell_np, cell_d = gpu_order(keys_d, counts_d, n, max_kp, H, W)
    assert R.reference_order_is_valid(cell_np, keys, counts, H, W), name
    shuf_d = _dev(shuffled_order(counts, max_kp, 5))
    runs = [("plain", img_d, blur_d, None), ("ordered", img_d, blur_d, cell_d), ("ordered", img_d, blur_d, shuf_d)]
    tiled = W % 16 == 0 and H % 8 == 0 and pitch == W
    if tiled:
        img_t, blur_t = tile_planes(img_d), tile_planes(blur_d)
        runs += [("tiled", img_t, blur_t, cell_d), ("tiled", img_t, blur_t, None)]
    for j, (entry, a, b, order_d) in enumerate(runs):
        if entries is not None and entry not in entries:
            continue
        desc, ang = run_entry(entry, a, b, keys_d, counts_d, order_d, n, H, W, pitch, max_kp)
        bad_a = np.argwhere(ang != ref["angle"])
        assert bad_a.size == 0, (name, entry, j, "angle", bad_a[:5].tolist(), ang[tuple(bad_a[0])], ref["angle"][tuple(bad_a[0])])
        bad_d = np.argwhere((desc != ref["desc"]).any(-1))
        assert bad_d.size == 0, (name, entry, j, "descriptor", bad_d[:5].tolist())
    # nothing the launches read has changed
    assert np.array_equal(img_d.cpu().numpy(), img) and np.array_equal(blur_d.cpu().numpy(), blur)
    assert np.array_equal(keys_d.cpu().numpy().view(np.uint32), keys) and np.array_equal(counts_d.cpu().numpy(), counts)
    assert np.array_equal(cell_d.cpu().numpy().reshape(n, max_kp), cell_np)
    if tiled:
        assert torch.equal(img_t, tile_planes(img_d)) and torch.equal(blur_t, tile_planes(blur_d))
    return tiled


@pytest.mark.parametrize("name", R.MOMENTS_CASES)
def test_bin_ties_flat_patches_and_every_bin(gpu, name):
    """All 30 exact ties of adjacent bins with the moments one unit either side (smallest and largest reachable
    magnitude), flat patches at 0, 1 and 255, the axis directions, every bin; ties at slot 0, slot 7 and in a lone live
    slot of a wave.  tests/test_orb_ref.py asserts that the cases hold these."""
    assert check_case("moments:" + name)


def test_saturated_half_discs_and_a_white_image(gpu):
    assert check_case("saturated")


@pytest.mark.parametrize("name", ["impulse", "impulse_complement"])
def test_single_pixel_planes_pin_the_rotated_offsets(gpu, name):
    """Every bin, 20 offsets each out of the bin's own table (the farthest in each direction among them): the expected
    words follow from the table alone, and n_img = 30 deals the images over the block map's eight lanes four times."""
    _, _, _, _, meta, ref = R.image_case(name)
    assert np.array_equal(ref["desc"], meta["expected"])
    assert check_case(name)


def test_planes_of_equal_values(gpu):
    """Constant planes (all bits 0), two-level checkerboards and ramps: bits decided by equality, a < b strict."""
    assert check_case("equal_planes")


@pytest.mark.parametrize("H,W,pitch", R.EVERY_PIXEL_SHAPES)
@pytest.mark.parametrize("order", ["raster", "shuffled"])
def test_every_pixel_is_a_keypoint(gpu, H, W, pitch, order):
    """Both sides of each fast-path condition of both patch loaders at every byte alignment (tests/test_orb_ref.py
    asserts it per shape); (20, 20) is never on the fast path; odd widths, an odd pitch and H * pitch % 4 != 0 take the
    exact-start instances; (48, 64) and (40, 48) run through the tiled entry point as well, (40, 48) being exactly one
    tiled descriptor patch row wide.  The library accepts all of these shapes as they are."""
    tiled = check_case(f"every_pixel:{H}x{W}p{pitch}:{order}")
    assert tiled == ((H, W, pitch) in R.EVERY_PIXEL_TILED_SHAPES)


@pytest.mark.parametrize("which", ["img", "blur"])
def test_a_base_pointer_off_the_dword_boundary(gpu, which):
    """The plane starts one byte into a larger device buffer: its rows are off dword boundaries although W and the pitch
    are multiples of 4, and the host must select the exact-start instances."""
    L = _L()
    img, blur, keys, counts, meta, ref = R.image_case("every_pixel:48x64p64:shuffled")
    H, W, pitch = meta["H"], meta["W"], meta["pitch"]
    n, max_kp = keys.shape
    planes = {}
    for nm, a in (("img", img), ("blur", blur)):
        if nm == which:
            buf = torch.full((a.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            buf[1:1 + a.size] = _dev(a).reshape(-1)
            planes[nm] = buf[1:1 + a.size]
            assert planes[nm].data_ptr() % 4 == 1
        else:
            planes[nm] = _dev(a)
            assert planes[nm].data_ptr() % 4 == 0
    keys_d, counts_d = _dev(keys.view(np.int32)), _dev(counts)
    _, cell_d = gpu_order(keys_d, counts_d, n, max_kp, H, W)
    for entry, order_d in (("plain", None), ("ordered", cell_d)):
        desc, ang = run_entry(entry, planes["img"], planes["blur"], keys_d, counts_d, order_d, n, H, W, pitch, max_kp)
        assert np.array_equal(ang, ref["angle"]) and np.array_equal(desc, ref["desc"]), entry
    assert np.array_equal(planes["img"].cpu().numpy().reshape(img.shape), img)
    assert np.array_equal(planes["blur"].cpu().numpy().reshape(blur.shape), blur)


@pytest.mark.parametrize("max_kp", R.COUNTS_MAX_KP)
@pytest.mark.parametrize("n_img", R.COUNTS_N_IMG)
def test_image_counts_and_keypoint_counts(gpu, n_img, max_kp):
    """n_img around the eight lanes of the block -> (image, chunk) map; counts below zero, zero, around the eight
    keypoints of a wave and the 32 of a workgroup, at and above max_kp; unused key slots VUS_KEY_INVALID."""
    check_case(f"counts:{n_img}:{max_kp}")


@pytest.mark.parametrize("name", R.ORDER_CASES)
def test_orient_order(gpu, name):
    """vus_orient_order alone (it reads no image): one cell, one keypoint per cell, empty and full lists, max_kp below the
    256 threads and at 8192, a width that is no multiple of 64, exactly 1024 cells; 1056 cells are refused with the
    library's error and the order is left untouched."""
    L = _L()
    _, _, keys, counts, meta = R.order_case(name)
    H, W, max_kp = meta["H"], meta["W"], meta["max_kp"]
    n = keys.shape[0]
    keys_d, counts_d = _dev(keys.view(np.int32)), _dev(counts)
    if meta["refused"]:
        order = torch.full((n, max_kp), ORDER_FILL, dtype=torch.int32, device="cuda")
        with pytest.raises(L.VusError, match="more than 1024 cells"):
            L.call("vus_orient_order", keys_d.data_ptr(), counts_d.data_ptr(), n, max_kp, H, W, order.data_ptr(), L.current_stream_ptr())
        torch.cuda.synchronize()
        assert (order == ORDER_FILL).all()
        return
    order, _ = gpu_order(keys_d, counts_d, n, max_kp, H, W)
    assert R.reference_order_is_valid(order, keys, counts, H, W)
    assert np.array_equal(keys_d.cpu().numpy().view(np.uint32), keys) and np.array_equal(counts_d.cpu().numpy(), counts)
