"""-m gpu: the kernels of csrc/boundary.hip through their `ops` wrappers, for exact equality with a host reference that follows the
definitions and shares no code with them: row packing bit by bit, and erosion by a summed-area table over the zero-padded mask
(eroded = the (2 d + 1)^2 window sum equals (2 d + 1)^2).  Then Boundary IoU of mask sets, the capture of the whole chain into a graph,
and Boundary AP end to end on the tiny fixture model's own masks.  Every comparison is integer or float64 equality."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 63), (3, 64), (3, 65), (5, 130), (70, 200)]
DILATIONS = [1, 2, 31, 32, 33, 63, 64, 65, 70]     # a shift inside a word, of one word, of more; 2 d + 1 below, at and above W and H


# ---------------------------------------------------------------------------------------------------- host reference
def ref_pack_rows(masks):
    """row-packed int64 [n, H * wpr] of host masks [n, H, W], by the definition: pixel (y, x) = bit x % 64 of word y * wpr + x // 64"""
    m = np.asarray(masks) != 0
    n, H, W = m.shape
    wpr = (W + 63) // 64
    padded = np.zeros((n, H, wpr * 64), dtype=np.uint64)
    padded[:, :, :W] = m
    words = (padded.reshape(n, H, wpr, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)     # disjoint bits: sum = or
    return torch.from_numpy(words.reshape(n, H * wpr).view(np.int64).copy()), torch.from_numpy(m.reshape(n, -1).sum(1).astype(np.int64))


def ref_erode(masks, d):
    """eroded[y, x] = 1 iff the (2 d + 1)^2 window around (y, x) lies inside the image and is all set: a summed-area table over the
    mask padded with d zeros on every side"""
    m = (np.asarray(masks) != 0).astype(np.int64)
    n, H, W = m.shape
    k = 2 * d + 1
    sat = np.zeros((n, H + 2 * d + 1, W + 2 * d + 1), dtype=np.int64)
    sat[:, d + 1: d + 1 + H, d + 1: d + 1 + W] = m
    sat = sat.cumsum(1).cumsum(2)
    window = sat[:, k:, k:] - sat[:, :-k, k:] - sat[:, k:, :-k] + sat[:, :-k, :-k]       # [n, H, W]: the sum of rows y - d .. y + d, ...
    return (window == k * k).astype(np.uint8)


def ref_boundary(masks, d):
    m = (np.asarray(masks) != 0).astype(np.uint8)
    return m & (1 - ref_erode(m, d))


def ref_inter(a, b):
    a, b = torch.from_numpy(np.asarray(a)).flatten(1).long(), torch.from_numpy(np.asarray(b)).flatten(1).long()
    return a @ b.T


def ref_iou(inter, area_a, area_b):
    union = area_a[:, None] + area_b[None, :] - inter
    return torch.where(union > 0, inter.double() / union.clamp_min(1).double(), torch.zeros((), dtype=torch.float64))


def blobs(n, H, W, seed):
    """n host masks uint8 [H, W] of values {0, 1}: smooth noise thresholded at different levels, so contours cross the image edges; mask 1
    also carries a frame along all four edges, mask 2 (if any) is full"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((n, 1, (H + 7) // 8 + 2, (W + 7) // 8 + 2), generator=g)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True)[:, 0]
    level = torch.tensor([0.35, 0.45, 0.0, 0.55, 0.5])[torch.arange(n) % 5]
    m = (field > level[:, None, None]).to(torch.uint8)
    if n > 1:
        t = max(1, min(H, W) // 10)
        m[1, :t] = 1
        m[1, -t:] = 1
        m[1, :, :t] = 1
        m[1, :, -t:] = 1
    if n > 2:
        m[2] = 1
    return m


def tile_of(H, W, d):
    """(rows, words) of the boundary kernel's tile on this device"""
    from ape_amd import _lib
    rows, words = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().ape_hip_bitmask_boundary_tile(H, W, d, 0, ctypes.byref(rows), ctypes.byref(words)) >= 0
    return rows.value, words.value


# ---------------------------------------------------------------------------------------------------- 1. row pack
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_rows_layout_area_unaligned_bases_and_unpack(hw):
    """values {0, 1, 2, 255} behind 0 .. 15 leading bytes of a buffer of foreground: layout, zero padding bits, area; unpack inverts pack
    and writes nothing outside its output, at every byte offset too"""
    from ape_amd import ops
    H, W = hw
    n = 3
    g = torch.Generator().manual_seed(H * 1000 + W)
    host = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (n, H, W), generator=g)]
    want_bits, want_area = ref_pack_rows(host.numpy())
    wpr = (W + 63) // 64
    want_bytes = (host != 0).to(torch.uint8)
    for off in range(16):
        buf = torch.full((off + n * H * W + 64,), 255, dtype=torch.uint8, device="cuda")          # foreground all around the masks
        buf[off: off + n * H * W] = host.reshape(-1).cuda()
        m = buf[off: off + n * H * W].view(n, H, W)
        assert m.data_ptr() == buf.data_ptr() + off
        bits, area = ops.mask_pack_rows(m)
        assert bits.dtype == torch.int64 and tuple(bits.shape) == (n, H * wpr) and area.dtype == torch.int64 and tuple(area.shape) == (n,)
        assert torch.equal(bits.cpu(), want_bits), (hw, off)
        assert torch.equal(area.cpu(), want_area), (hw, off)
        if W % 64:                                              # the unused high bits of every row's last word are zero
            last = bits.view(n, H, wpr)[:, :, -1].cpu()
            assert int(((last >> (W % 64)) != 0).sum()) == 0
        out_buf = torch.full((off + n * H * W + 37,), 0xAB, dtype=torch.uint8, device="cuda")
        out = out_buf[off: off + n * H * W].view(n, H, W)
        assert ops.bitmask_unpack_rows(bits, H, W, out=out) is out
        back = out_buf.cpu()
        assert int((back[:off] != 0xAB).sum()) == 0 and int((back[off + n * H * W:] != 0xAB).sum()) == 0, (hw, off)
        assert torch.equal(back[off: off + n * H * W].view(n, H, W), want_bytes), (hw, off)
    assert torch.equal(ops.bitmask_unpack_rows(ops.mask_pack_rows(host.bool().cuda())[0], H, W).cpu(), want_bytes)      # bool storage
    bits, area = ops.mask_pack_rows(torch.zeros((0, H, W), dtype=torch.uint8, device="cuda"))
    assert tuple(bits.shape) == (0, H * wpr) and tuple(area.shape) == (0,)
    assert tuple(ops.bitmask_unpack_rows(bits, H, W).shape) == (0, H, W)


def test_pack_rows_more_rows_than_a_grid_has_rows():
    """100 masks of 700 rows are 70 000 rows of two words: more than the 65 535 masks one mask_pack_bits call takes"""
    from ape_amd import ops
    m = blobs(5, 700, 65, 3).repeat(20, 1, 1)
    bits, area = ops.mask_pack_rows(m.cuda())
    want_bits, want_area = ref_pack_rows(m.numpy())
    assert torch.equal(bits.cpu(), want_bits) and torch.equal(area.cpu(), want_area)


# ---------------------------------------------------------------------------------------------------- 2. boundary against the reference
_CASES = {}


def _case(hw):
    """the masks of one shape, packed by the reference and uploaded once"""
    if hw not in _CASES:
        H, W = hw
        host = blobs(5, H, W, 7 * H + W).numpy()
        _CASES[hw] = (host, ref_pack_rows(host)[0].cuda())
    return _CASES[hw]


def _check_boundary(host, bits, H, W, d):
    from ape_amd import ops
    band = ref_boundary(host, d)
    want_bits, want_area = ref_pack_rows(band)
    bbits, barea = ops.bitmask_boundary(bits, H, W, d)
    assert bbits.dtype == torch.int64 and tuple(bbits.shape) == tuple(bits.shape) and barea.dtype == torch.int64
    wrong = int((bbits.cpu() != want_bits).sum())
    assert wrong == 0, ((H, W), d, wrong)
    assert torch.equal(barea.cpu(), want_area), ((H, W), d)
    return band


@pytest.mark.parametrize("d", DILATIONS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundary_equals_the_reference(hw, d):
    host, bits = _case(hw)
    _check_boundary(host, bits, hw[0], hw[1], d)


@pytest.mark.parametrize("d", [31, 32, 33, 64, 65, 70, 99])
def test_boundary_wide_bands_inside_a_larger_image(d):
    """200 x 200 keeps 2 d + 1 <= H, W up to d = 99, so the erosion itself runs (not the band-is-the-mask case) with horizontal runs of
    more than 64 and more than 128 bits: windows that span two and three neighbouring words"""
    host, bits = _case((200, 200))
    assert tile_of(200, 200, d)[0] > 0
    band = _check_boundary(host, bits, 200, 200, d)
    assert int(band[2].sum()) == 200 * 200 - (200 - 2 * d) ** 2          # the full mask


# ---------------------------------------------------------------------------------------------------- 3. known answers
@pytest.mark.parametrize("hw", [(5, 130), (70, 200), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundary_known_answers(hw):
    from ape_amd import ops
    H, W = hw
    for d in (1, 2, 7, 33):
        ones = torch.ones((1, H, W), dtype=torch.uint8, device="cuda")
        bits, area = ops.mask_pack_rows(ones)
        _, barea = ops.bitmask_boundary(bits, H, W, d)
        assert int(area[0]) == H * W and int(barea[0]) == H * W - max(H - 2 * d, 0) * max(W - 2 * d, 0), (hw, d)
        zbits, _ = ops.mask_pack_rows(torch.zeros((2, H, W), dtype=torch.uint8, device="cuda"))
        zb, zarea = ops.bitmask_boundary(zbits, H, W, d)
        assert int(zb.abs().sum()) == 0 and zarea.tolist() == [0, 0]
        # one cleared pixel: exactly the clipped (2 d + 1)^2 square around it joins the frame of width d, without the pixel itself
        y0, x0 = H // 2, W // 2 + 1
        holed = ones.clone()
        holed[0, y0, x0] = 0
        band = ops.mask_boundary(holed, dilation=d).cpu()[0]
        want = torch.ones((H, W), dtype=torch.uint8)
        if H > 2 * d and W > 2 * d:
            want[d: H - d, d: W - d] = 0
        want[max(y0 - d, 0): y0 + d + 1, max(x0 - d, 0): x0 + d + 1] = 1
        want[y0, x0] = 0
        assert torch.equal(band, want), (hw, d)
        # a rectangle flush with the top left corner erodes on the flush sides too: what is left is its own frame of width d
        h, w = min(H, 4 * d + 3), min(W, 4 * d + 5)
        rect = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
        rect[0, :h, :w] = 1
        band = ops.mask_boundary(rect, dilation=d).cpu()[0]
        want = torch.zeros((H, W), dtype=torch.uint8)
        want[:h, :w] = 1
        if h > 2 * d and w > 2 * d:
            want[d: h - d, d: w - d] = 0
        assert torch.equal(band, want), (hw, d)
    assert torch.equal(ops.mask_boundary(ones), ops.mask_boundary(ones, dilation=ops.boundary_dilation(H, W)))     # the default width


# ---------------------------------------------------------------------------------------------------- 4. tile edges
# (700, 65), d = 3   : a tile is 64 rows (the 4 d wanted rows are at least 64) by both words -> 11 row tiles, the last of 60 rows
# (9, 4200), d = 3   : 66 words per row, a word tile is at most 32 words -> 3 word tiles, the last of 2 words, one row tile
# (400, 4200), d = 66: 2 d = 132 halo rows leave room for 8-word tiles only -> 2 row tiles x 9 word tiles, and the horizontal run of 133
#                      bits reaches two words to either side, across word-tile edges
# (700, 65), d = 66 and (9, 4200), d = 66: 2 d + 1 exceeds W or H, the band is the mask (no tile)
@pytest.mark.parametrize("case", [(700, 65, 3, True, False), (9, 4200, 3, False, True), (400, 4200, 66, True, True), (700, 65, 66, None, None),
                                  (9, 4200, 66, None, None)], ids=lambda c: f"{c[0]}x{c[1]}-d{c[2]}")
def test_boundary_across_row_tiles_and_word_tiles(case):
    H, W, d, many_rows, many_words = case
    rows, words = tile_of(H, W, d)
    if many_rows is None:
        assert (rows, words) == (0, 0)
    else:
        assert (rows < H) == many_rows and (words < (W + 63) // 64) == many_words, (rows, words)
    host = blobs(3, H, W, H + W + d).numpy()
    _check_boundary(host, ref_pack_rows(host)[0].cuda(), H, W, d)


# ---------------------------------------------------------------------------------------------------- 5. pairs
@pytest.mark.parametrize("nm", [(1, 1), (3, 2), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundary_pair_iou_equals_the_reference(nm):
    from ape_amd import ops
    n, m = nm
    H, W = 70, 200
    d = ops.boundary_dilation(H, W)
    assert d == 4
    a, b = blobs(n, H, W, 31 * n + m), blobs(m, H, W, 37 * n + m)
    if n > 1:
        a[0] = 0                                                # an empty mask on either side: its pairs have empty unions
        b[0] = 0
    res = ops.boundary_pair_iou(a.cuda(), (b * 255).cuda())
    biou, iou, binter, inter, barea_a, barea_b, area_a, area_b = (t.cpu() for t in res)
    band_a, band_b = ref_boundary(a.numpy(), d), ref_boundary(b.numpy(), d)
    want_inter, want_binter = ref_inter(a.numpy(), b.numpy()), ref_inter(band_a, band_b)
    wa, wb = a.flatten(1).long().sum(1), b.flatten(1).long().sum(1)
    wba, wbb = torch.from_numpy(band_a.reshape(n, -1).sum(1).astype(np.int64)), torch.from_numpy(band_b.reshape(m, -1).sum(1).astype(np.int64))
    assert all(t.dtype == torch.int64 for t in (binter, inter, barea_a, barea_b, area_a, area_b))
    assert torch.equal(inter, want_inter) and torch.equal(binter, want_binter)
    assert torch.equal(area_a, wa) and torch.equal(area_b, wb) and torch.equal(barea_a, wba) and torch.equal(barea_b, wbb)
    assert biou.dtype == torch.float64 and iou.dtype == torch.float64 and tuple(biou.shape) == (n, m)
    assert torch.equal(iou, ref_iou(want_inter, wa, wb)) and torch.equal(biou, ref_iou(want_binter, wba, wbb))
    if n > 1:
        assert float(biou[0, 0]) == 0.0 and float(iou[0, 0]) == 0.0 and float(biou[0].abs().sum()) == 0.0
    wide = ops.boundary_pair_iou(a.cuda(), b.cuda(), dilation=9)[0].cpu()
    ratio = ops.boundary_pair_iou(a.cuda(), b.cuda(), dilation_ratio=9.0 / 211.0)[0].cpu()
    band_a, band_b = ref_boundary(a.numpy(), 9), ref_boundary(b.numpy(), 9)
    want = ref_iou(ref_inter(band_a, band_b), torch.from_numpy(band_a.reshape(n, -1).sum(1).astype(np.int64)),
                   torch.from_numpy(band_b.reshape(m, -1).sum(1).astype(np.int64)))
    assert torch.equal(wide, want) and torch.equal(ratio, want)


def test_boundary_pair_iou_of_empty_sets():
    from ape_amd import ops
    none = torch.zeros((0, 5, 130), dtype=torch.uint8, device="cuda")
    some = torch.ones((2, 5, 130), dtype=torch.uint8, device="cuda")
    res = ops.boundary_pair_iou(none, some)
    assert tuple(res[0].shape) == (0, 2) and tuple(res[1].shape) == (0, 2) and tuple(res[4].shape) == (0,) and tuple(res[5].shape) == (2,)
    res = ops.boundary_pair_iou(some, none)
    assert tuple(res[0].shape) == (2, 0) and tuple(res[3].shape) == (2, 0)
    assert tuple(ops.mask_boundary(none).shape) == (0, 5, 130)


# ---------------------------------------------------------------------------------------------------- 6. wrappers
def test_wrappers_reject_wrong_inputs():
    from ape_amd import ops
    m = torch.zeros((2, 6, 70), dtype=torch.uint8, device="cuda")
    bits, _ = ops.mask_pack_rows(m)
    assert tuple(bits.shape) == (2, 12)
    with pytest.raises(TypeError):
        ops.mask_pack_rows(m.int())
    with pytest.raises(ValueError):
        ops.mask_pack_rows(m[0])                                                    # rank
    with pytest.raises(ValueError):
        ops.mask_pack_rows(m.transpose(1, 2))                                       # not contiguous
    with pytest.raises(RuntimeError):
        ops.mask_pack_rows(m.cpu())
    with pytest.raises(TypeError):
        ops.bitmask_boundary(bits.int(), 6, 70, 1)
    with pytest.raises(ValueError):
        ops.bitmask_boundary(bits, 6, 70, 0)                                        # d < 1
    with pytest.raises(ValueError):
        ops.bitmask_boundary(bits, 6, 64, 1)                                        # 6 rows of 64 pixels are 6 words, not 12
    with pytest.raises(ValueError):
        ops.bitmask_boundary(bits, 0, 70, 1)
    with pytest.raises(ValueError):
        ops.bitmask_boundary(bits.reshape(2, 6, 2), 6, 70, 1)                       # rank
    with pytest.raises(ValueError):
        ops.bitmask_boundary(bits.t(), 6, 70, 1)                                    # not contiguous
    with pytest.raises(TypeError):
        ops.bitmask_unpack_rows(bits.double(), 6, 70)
    with pytest.raises(ValueError):
        ops.bitmask_unpack_rows(bits, 7, 70)
    with pytest.raises(ValueError):
        ops.bitmask_unpack_rows(bits, 6, 70, out=torch.zeros((2, 70, 6), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.mask_boundary(m, dilation=0)
    with pytest.raises(TypeError):
        ops.mask_boundary(m.float())
    with pytest.raises(ValueError):
        ops.boundary_pair_iou(m, m[:, :, :69].contiguous())                         # sizes differ
    with pytest.raises(ValueError):
        ops.boundary_pair_iou(m, m, dilation=-1)
    with pytest.raises(TypeError):
        ops.boundary_pair_iou(m, m.long())


# ---------------------------------------------------------------------------------------------------- 7. graph capture
def test_the_whole_chain_captures_into_a_graph():
    """both packs, both boundaries and both pair counts on one stream (200 x 333 masks are 1200 words: the pair counts split the word axis
    and zero their outputs with memset nodes, like the areas and band areas): capturing runs nothing, and two replays on different inputs
    written into the static buffers are each correct"""
    from ape_amd import ops
    H, W, d = 200, 333, 5
    inputs = [(blobs(5, H, W, 21), blobs(3, H, W, 22)), (blobs(5, H, W, 23), blobs(3, H, W, 24))]
    a, b = inputs[0][0].cuda(), inputs[0][1].cuda()
    ops.boundary_pair_iou(a, b, dilation=d)                     # warm: nothing is set up lazily inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a_bits, area_a = ops.mask_pack_rows(a)
        b_bits, area_b = ops.mask_pack_rows(b)
        a_band, barea_a = ops.bitmask_boundary(a_bits, H, W, d)
        b_band, barea_b = ops.bitmask_boundary(b_bits, H, W, d)
        inter = ops.bitmask_pair_counts(a_bits, b_bits)
        binter = ops.bitmask_pair_counts(a_band, b_band)
    torch.cuda.synchronize()
    for t in (inter, binter, area_a, barea_a, barea_b):
        t.fill_(-7)
    torch.cuda.synchronize()
    assert int(binter[0, 0]) == -7 and int(barea_a[0]) == -7                   # capturing did not run the kernels
    for ha, hb in (inputs[1], inputs[0]):
        a.copy_(ha.cuda())
        b.copy_(hb.cuda())
        graph.replay()
        torch.cuda.synchronize()
        band_a, band_b = ref_boundary(ha.numpy(), d), ref_boundary(hb.numpy(), d)
        assert torch.equal(inter.cpu(), ref_inter(ha.numpy(), hb.numpy())) and torch.equal(binter.cpu(), ref_inter(band_a, band_b))
        assert torch.equal(area_a.cpu(), ha.flatten(1).long().sum(1)) and torch.equal(area_b.cpu(), hb.flatten(1).long().sum(1))
        assert barea_a.cpu().tolist() == band_a.reshape(5, -1).sum(1).tolist() and barea_b.cpu().tolist() == band_b.reshape(3, -1).sum(1).tolist()


# ---------------------------------------------------------------------------------------------------- 8. end to end
def test_boundary_ap_on_the_models_own_masks():
    """the tiny panoptic fixture's instances (built as tests/test_mask_iou_gpu.py builds them): against themselves Boundary AP is 1.0;
    against themselves rolled by 2 pixels it is exactly the protocol on min(mask IoU, boundary IoU) of the host reference; byte masks,
    RLE dicts and an Instances carrying pred_masks_rle give the same result"""
    import model_util as M
    from ape_amd import ops
    from ape_amd.evaluation import BoundaryAPAccumulator, _coco_ap, boundary_ap, boundary_iou, encode_masks
    from ape_amd.structures import Instances

    model, image, text, gold = M.build_model("tiny_panoptic", device="cuda", dtype=torch.float32)
    mv = model.model_vision
    meta = gold["semantic_meta"]
    mv.dataset_names, mv.dataset_name_to_idx, mv.dataset_prompts = ["coco"], {"coco": 0}, ["name"]
    mv.set_metadata(0, name="coco_2017_val", thing_classes=meta["thing_classes"], stuff_classes=meta["stuff_classes"],
                    thing_dataset_id_to_contiguous_id={i + 1: i for i in range(len(meta["thing_classes"]))})
    mv.semantic_on = mv.panoptic_on = True
    mv.panoptic_configs = dict(gold["panoptic_cfg"])
    mv.set_model_language(M.TextStub(text.cuda()))
    mv.set_eval_dataset("coco_2017_val")
    H, W = gold["out_hw"]
    inst = model([{"image": image.cuda(), "height": H, "width": W}])[0]["instances"]
    masks = inst.pred_masks.cuda()
    keep = (masks.flatten(1).sum(1) > 0).nonzero().flatten()
    assert keep.numel() > 1 and tuple(masks.shape[1:]) == (H, W)
    masks, scores, classes = masks[keep].contiguous(), inst.scores.cuda()[keep], inst.pred_classes.cuda()[keep]
    # identical masks of one class would compete for each other's ground truth in any order: keep one of each
    iou = ops.mask_pair_iou(masks, masks)[0]
    same = (iou.cpu() == 1.0) & (classes.cpu()[:, None] == classes.cpu()[None, :])
    first = torch.tensor([int(same[i].nonzero()[0]) == i for i in range(len(keep))])
    masks, scores, classes = masks[first.cuda()].contiguous(), scores[first.cuda()], classes[first.cuda()]
    masks = masks.ne(0).to(torch.uint8)
    assert boundary_ap([(masks, scores, classes)], [(masks, classes)])["AP"] == 1.0
    assert float(boundary_iou(masks, masks).diagonal().min()) == 1.0

    gt = torch.roll(masks, 2, dims=2).contiguous()
    d = ops.boundary_dilation(H, W)
    hm, hg = masks.cpu().numpy(), gt.cpu().numpy()
    bm, bg = ref_boundary(hm, d), ref_boundary(hg, d)
    area = lambda x: torch.from_numpy(x.reshape(x.shape[0], -1).sum(1).astype(np.int64))     # noqa: E731
    host_iou = ref_iou(ref_inter(hm, hg), area(hm), area(hg))
    host_biou = ref_iou(ref_inter(bm, bg), area(bm), area(bg))
    assert torch.equal(boundary_iou(masks, gt).cpu(), host_biou)
    want = _coco_ap([(scores.cpu().double(), classes.cpu(), classes.cpu(), torch.minimum(host_iou, host_biou))])
    got = boundary_ap([(masks, scores, classes)], [(gt, classes)])
    assert got == want and got["gt"] == masks.shape[0]
    rles = encode_masks(masks)
    assert boundary_ap([(rles, scores, classes)], [(encode_masks(gt), classes)]) == want      # RLE dicts on both sides
    assert boundary_ap([(masks.bool().cpu(), scores, classes)], [(gt.cpu(), classes)]) == want         # host tensors, bool storage
    acc = BoundaryAPAccumulator()
    carrier = Instances((H, W))
    carrier.scores, carrier.pred_classes, carrier.pred_masks_rle = scores, classes, rles
    acc.update(carrier, gt_masks=gt, gt_classes=classes)
    assert acc.compute() == want
    other = boundary_ap([(masks, scores, classes)], [(gt, classes)], dilation_ratio=0.1)
    bm, bg = ref_boundary(hm, ops.boundary_dilation(H, W, 0.1)), ref_boundary(hg, ops.boundary_dilation(H, W, 0.1))
    assert other == _coco_ap([(scores.cpu().double(), classes.cpu(), classes.cpu(),
                               torch.minimum(host_iou, ref_iou(ref_inter(bm, bg), area(bm), area(bg))))])
