"""-m gpu: the kernels of csrc/maskiou.hip through their `ops` wrappers, for exact equality with host integer arithmetic
(`a.bool().flatten(1).long() @ b.bool().flatten(1).long().T` and `.sum`): the bit pack, the pair counts, their capture into a graph,
`rle_decode` as the inverse of `rle_encode`, and mask AP end to end on the tiny fixture model's own masks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (3, 21), (8, 8), (5, 13), (37, 53), (64, 64), (200, 333)]      # word, wave and vector boundaries, non-zero tails


def host_bits(masks):
    """(bits int64 [n, words], area) of host masks: pixel p = bit p % 64 of word p // 64"""
    n = masks.shape[0]
    flat = (masks.reshape(n, -1) != 0).long()
    words = (flat.shape[1] + 63) // 64
    padded = torch.zeros((n, words * 64), dtype=torch.int64)
    padded[:, : flat.shape[1]] = flat
    weight = torch.tensor([1 << k for k in range(63)] + [-(1 << 63)], dtype=torch.int64)
    return (padded.reshape(n, words, 64) * weight).sum(-1), flat.sum(1)


def host_inter(a, b):
    return a.cpu().bool().flatten(1).long() @ b.cpu().bool().flatten(1).long().T


def _values(shape, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "bool":
        return torch.rand(shape, generator=g) < 0.4
    return torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, shape, generator=g)]


# ---------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_bits_layout_area_and_unaligned_bases(hw):
    """values {0, 1, 2, 255} and bool storage; the base 0 and 1 masks into a larger buffer (an odd H * W then gives an odd byte address)"""
    from ape_amd import ops
    H, W = hw
    for kind in ("u8", "bool"):
        buf = _values((4, H, W), H * 1000 + W + (kind == "bool"), kind)
        dev = buf.cuda()
        for first in (0, 1):
            m = dev[first:]
            assert m.is_contiguous() and m.data_ptr() == dev.data_ptr() + first * H * W
            bits, area = ops.mask_pack_bits(m)
            want_bits, want_area = host_bits(buf[first:])
            assert bits.dtype == torch.int64 and tuple(bits.shape) == (4 - first, (H * W + 63) // 64) and area.dtype == torch.int64
            assert torch.equal(bits.cpu(), want_bits), (hw, kind, first)
            assert torch.equal(area.cpu(), want_area)
            tail = (H * W) % 64
            if tail:                                            # the unused high bits of the last word are zero
                assert int(((bits[:, -1].cpu() >> tail) != 0).sum()) == 0
    bits, area = ops.mask_pack_bits(torch.zeros((0, H, W), dtype=torch.uint8, device="cuda"))
    assert tuple(bits.shape) == (0, (H * W + 63) // 64) and tuple(area.shape) == (0,)


def test_pack_every_byte_offset_of_a_vector():
    """the same 3 x (37 x 53) masks behind 0 .. 16 leading bytes: every misalignment of the base against the 16-byte loads"""
    from ape_amd import ops
    n, H, W = 3, 37, 53
    host = _values((n, H, W), 7, "u8")
    want_bits, want_area = host_bits(host)
    for off in range(17):
        buf = torch.full((off + n * H * W + 64,), 255, dtype=torch.uint8, device="cuda")      # foreground all around the masks
        buf[off: off + n * H * W] = host.reshape(-1).cuda()
        m = buf[off: off + n * H * W].view(n, H, W)
        bits, area = ops.mask_pack_bits(m)
        assert torch.equal(bits.cpu(), want_bits) and torch.equal(area.cpu(), want_area), off


# ---------------------------------------------------------------------------------------------------- pair counts
def _iou_check(a, b):
    from ape_amd import ops
    iou, inter, area_a, area_b = ops.mask_pair_iou(a, b)
    want = host_inter(a, b)
    wa, wb = a.cpu().bool().flatten(1).long().sum(1), b.cpu().bool().flatten(1).long().sum(1)
    assert inter.dtype == torch.int64 and torch.equal(inter.cpu(), want), int((inter.cpu() != want).sum())
    assert torch.equal(area_a.cpu(), wa) and torch.equal(area_b.cpu(), wb)
    union = wa[:, None] + wb[None, :] - want
    want_iou = torch.where(union > 0, want.double() / union.clamp_min(1).double(), torch.zeros((), dtype=torch.float64))
    assert iou.dtype == torch.float64 and torch.equal(iou.cpu(), want_iou)
    return inter


@pytest.mark.parametrize("nm", [(1, 1), (1, 5), (3, 2), (17, 33), (70, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_counts_cross_every_tile_edge(nm):
    """64 x 64 tiles of pairs: one partial tile, a full one plus a remainder on either side; 37 x 53 masks are 31 words, less than one
    staging step of 32, 200 x 333 are 1041 words, a split word axis with a remainder"""
    n, m = nm
    for (H, W) in ((37, 53), (200, 333)) if n * m < 1000 else ((37, 53),):
        a = _values((n, H, W), 11 * n + m, "u8").cuda()
        b = _values((m, H, W), 13 * n + m, "bool").cuda()
        _iou_check(a, b)


def test_pair_counts_all_zero_all_one_and_counts_past_16_bits():
    z = torch.zeros((3, 37, 53), dtype=torch.uint8, device="cuda")
    o = torch.ones((2, 37, 53), dtype=torch.uint8, device="cuda")
    assert int(_iou_check(z, o).sum()) == 0
    assert _iou_check(o, o).tolist() == [[37 * 53] * 2] * 2
    big = torch.ones((2, 300, 400), dtype=torch.uint8, device="cuda")
    assert _iou_check(big, big[:1]).tolist() == [[120_000]] * 2               # does not fit 16 bits
    empty = torch.zeros((0, 37, 53), dtype=torch.uint8, device="cuda")
    from ape_amd import ops
    iou, inter, _, _ = ops.mask_pair_iou(empty, o)
    assert tuple(iou.shape) == (0, 2) and tuple(inter.shape) == (0, 2)


def test_pair_counts_long_word_axis_and_out_is_overwritten():
    """512 x 512 masks are 4096 words: with 3 x 2 pairs the word axis is split over the whole device (each split a multiple of 32 words),
    and the partial sums meet in atomics on a matrix the call itself zeroes -- a second call into the same `out` gives the same result"""
    from ape_amd import ops
    a = _values((3, 512, 512), 1, "u8").cuda()
    b = _values((2, 512, 512), 2, "bool").cuda()
    want = host_inter(a, b)
    _iou_check(a, b)
    a_bits, _ = ops.mask_pack_bits(a)
    b_bits, _ = ops.mask_pack_bits(b)
    out = torch.full((3, 2), 2 ** 40, dtype=torch.int64, device="cuda")
    for _ in range(2):
        assert ops.bitmask_pair_counts(a_bits, b_bits, out=out) is out
        assert torch.equal(out.cpu(), want)
    small = torch.full((3, 2), 2 ** 40, dtype=torch.int64, device="cuda")       # one staging step: the unsplit path stores, it does not add
    for _ in range(2):
        ops.bitmask_pair_counts(a_bits[:, :16].contiguous(), b_bits[:, :16].contiguous(), out=small)
        assert torch.equal(small.cpu(), host_inter(a[:, :2], b[:, :2]))         # 16 words = the first two rows of 512 pixels
    nothing = ops.bitmask_pair_counts(a_bits[:, :0].contiguous(), b_bits[:, :0].contiguous(), out=small)
    assert int(nothing.abs().sum()) == 0                                        # words == 0 writes zeros


def test_wrappers_reject_wrong_inputs():
    from ape_amd import ops
    m = torch.zeros((2, 6, 10), dtype=torch.uint8, device="cuda")
    bits, _ = ops.mask_pack_bits(m)
    with pytest.raises(TypeError):
        ops.mask_pack_bits(m.int())
    with pytest.raises(ValueError):
        ops.mask_pack_bits(m.transpose(1, 2))
    with pytest.raises(ValueError):
        ops.mask_pair_iou(m, m[:, :, :9].contiguous())
    with pytest.raises(TypeError):
        ops.bitmask_pair_counts(bits.int(), bits)
    with pytest.raises(ValueError):
        ops.bitmask_pair_counts(bits, torch.zeros((2, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.bitmask_pair_counts(bits, bits, out=torch.zeros((2, 2), dtype=torch.int32, device="cuda"))
    counts, nruns = ops.rle_encode(m, cap=8)
    with pytest.raises(TypeError):
        ops.rle_decode(counts.long(), nruns, 6, 10)
    with pytest.raises(ValueError):
        ops.rle_decode(counts, nruns[:1], 6, 10)
    with pytest.raises(ValueError):
        ops.rle_decode(counts, nruns, 6, 10, out=torch.zeros((2, 10, 6), dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------------- graph capture
def test_pack_and_pair_counts_capture_into_a_graph():
    """a single-branch graph of two packs and the pair counts (the split path, with its memset nodes): capturing runs nothing, two
    replays leave exactly the single-run result"""
    from ape_amd import ops
    a = _values((5, 200, 333), 21, "u8").cuda()
    b = _values((3, 200, 333), 22, "u8").cuda()
    want = host_inter(a, b)
    assert torch.equal(ops.mask_pair_iou(a, b)[1].cpu(), want)                  # warm: nothing is set up lazily inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a_bits, area_a = ops.mask_pack_bits(a)
        b_bits, area_b = ops.mask_pack_bits(b)
        inter = ops.bitmask_pair_counts(a_bits, b_bits)
    torch.cuda.synchronize()
    inter.fill_(-7)
    area_a.fill_(-7)
    torch.cuda.synchronize()
    assert int(inter[0, 0]) == -7                                               # capturing did not run the kernels
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(inter.cpu(), want)
    assert torch.equal(area_a.cpu(), a.cpu().bool().flatten(1).long().sum(1)) and torch.equal(area_b.cpu(), b.cpu().bool().flatten(1).long().sum(1))


# ---------------------------------------------------------------------------------------------------- RLE
def _blobs(n, H, W, seed):
    """random blobs: thresholded smooth noise, so the runs are neither single pixels nor whole columns"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((n, 1, (H + 3) // 4 + 1, (W + 3) // 4 + 1), generator=g)
    return (torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[:, 0] > 0.5).to(torch.uint8)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rle_decode_inverts_rle_encode(hw):
    from ape_amd import ops
    H, W = hw
    m = _blobs(6, H, W, H * 100 + W)
    m[1] = 0                                                    # the empty mask
    m[2] = 1                                                    # the full mask
    m[3, 0, 0] = 1                                              # first pixel foreground: an empty first run
    m[4] = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2).to(torch.uint8)      # checkerboard: H * W runs
    d = (m * 255).cuda()                                        # any non-zero value is foreground; the decoded mask holds 0 / 1
    counts, nruns = ops.rle_encode(d, cap=H * W + 1)
    assert int(nruns.max()) <= H * W + 1
    back = ops.rle_decode(counts, nruns, H, W)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (6, H, W) and torch.equal(back.cpu(), m)
    assert int(counts[3, 0]) == 0 and int(nruns[1]) == 1


def test_rle_decode_known_answer_clipping_and_guard_bytes():
    from ape_amd import ops
    counts = torch.tensor([[1, 3]], dtype=torch.int32, device="cuda")
    nruns = torch.tensor([2], dtype=torch.int32, device="cuda")
    assert ops.rle_decode(counts, nruns, 2, 2).tolist() == [[[0, 1], [1, 1]]]
    assert ops.rle_encode(torch.tensor([[[0, 1], [1, 1]]], dtype=torch.uint8, device="cuda"), cap=4)[0][0, :2].tolist() == [1, 3]
    # runs short of H * W leave zeros; a run past H * W is clipped (the second mask's 2^32 - 1 is -1 in int32 storage); runs after it add nothing
    counts = torch.tensor([[2, 3, 0, 0], [1, 2, 3, -1], [4, -1, 5, 5]], dtype=torch.int32, device="cuda")
    nruns = torch.tensor([2, 4, 4], dtype=torch.int32, device="cuda")
    H, W = 3, 5                                                 # column-major positions 0 .. 14
    want = torch.zeros((3, 15), dtype=torch.uint8)
    want[0, 2:5] = 1
    want[1, 1:3] = 1
    want[1, 6:] = 1
    want[2, 4:] = 1
    want = want.reshape(3, W, H).transpose(1, 2).contiguous()
    assert torch.equal(ops.rle_decode(counts, nruns, H, W).cpu(), want)
    # nruns > cap (a truncated encoding): the cap runs are decoded, the remainder is 0, and nothing outside `out` is written -- at an odd
    # byte address inside a buffer of guard bytes
    H, W = 37, 53
    m = _blobs(3, H, W, 5).cuda()
    cap = 24
    counts, nruns = ops.rle_encode(m, cap=cap)
    assert int(nruns.max()) > cap
    full_counts, full_nruns = ops.rle_encode(m, cap=H * W + 1)
    for lead in (16, 21):
        buf = torch.full((lead + 3 * H * W + 37,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[lead: lead + 3 * H * W].view(3, H, W)
        assert ops.rle_decode(counts, nruns, H, W, out=out) is out
        host = buf.cpu()
        assert int((host[:lead] != 0xAB).sum()) == 0 and int((host[lead + 3 * H * W:] != 0xAB).sum()) == 0
        for i in range(3):
            covered = int(full_counts[i, :cap].sum()) if int(full_nruns[i]) > cap else H * W
            got = host[lead + i * H * W: lead + (i + 1) * H * W].view(H, W).t().reshape(-1)          # column-major order
            ref = m[i].cpu().t().reshape(-1)
            assert torch.equal(got[:covered], ref[:covered]) and int(got[covered:].sum()) == 0, (lead, i)


# ---------------------------------------------------------------------------------------------------- end to end
def test_mask_ap_on_the_models_own_masks():
    """the tiny panoptic fixture's instances scored against themselves: AP 1.0; with the classes shifted by one: 0.0; the same masks
    through encode_masks -> decode_masks: identical masks, identical IoUs, and the accumulator takes the Instances as they are"""
    import model_util as M
    from ape_amd import ops
    from ape_amd.evaluation import MaskAPAccumulator, decode_masks, encode_masks, mask_ap

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
    iou, inter, area, _ = ops.mask_pair_iou(masks, masks)
    assert torch.equal(inter.cpu(), host_inter(masks, masks)) and torch.equal(inter.diagonal(), area)
    same = (iou.cpu() == 1.0) & (classes.cpu()[:, None] == classes.cpu()[None, :])
    first = torch.tensor([int(same[i].nonzero()[0]) == i for i in range(len(keep))])
    masks, scores, classes = masks[first.cuda()].contiguous(), scores[first.cuda()], classes[first.cuda()]
    assert mask_ap([(masks, scores, classes)], [(masks, classes)])["AP"] == 1.0
    # classes shifted by one.  The fixture's masks overlap across classes, so a detection relabelled c + 1 may rightly match an overlapping
    # ground truth whose class is c + 1 (measured: AP 0.197, not 0).  Two checks instead of one weaker one: in a vocabulary where a shift by one
    # can never meet a ground-truth class (even numbers) the AP is exactly 0.0, and with the raw shift it is exactly what the protocol gives
    # on the IoU matrix of host integer arithmetic
    assert mask_ap([(masks, scores, 2 * classes + 1)], [(masks, 2 * classes)])["AP"] == 0.0
    from ape_amd.evaluation import _coco_ap
    hi = host_inter(masks, masks)
    ha = hi.diagonal()
    host_iou = hi.double() / (ha[:, None] + ha[None, :] - hi).double()
    shifted = mask_ap([(masks, scores, classes + 1)], [(masks, classes)])
    assert shifted == _coco_ap([(scores.cpu().double(), classes.cpu() + 1, classes.cpu(), host_iou)]) and shifted["AP"] < 1.0
    rles = encode_masks(masks, cap=64)                          # a small cap: the truncated ones are encoded again with a larger one
    back = decode_masks(rles)
    assert back.is_cuda and torch.equal(back, masks.view(torch.uint8) if masks.dtype == torch.bool else masks.ne(0).to(torch.uint8))
    assert torch.equal(ops.mask_pair_iou(back, masks)[0], ops.mask_pair_iou(masks, masks)[0])
    assert mask_ap([(rles, scores, classes)], [(masks.cpu(), classes)])["AP"] == 1.0            # RLE dicts against a host tensor
    acc = MaskAPAccumulator()
    acc.update(inst, gt_masks=masks, gt_classes=classes)        # the Instances as the model returns them, all detections
    r = acc.compute()
    assert r["gt"] == int(first.sum()) and r["dets"] == len(inst) and 0.0 < r["AP"] <= 1.0
