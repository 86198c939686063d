"""The backbones' launch sequence, pinned on the CPU: which ops a backbone calls, in which order, with which shapes / dtypes /
strides / scalars, and where a parallel branch (ops.fork) opens, closes and is joined.  The numerical tests do not notice a launch
that is added, dropped, reordered or moved onto / off a forked branch -- on the GPU that is a silent change of speed or of the
captured graph's topology.  tests/golden/backbone_trace.json holds the sequences; APE_WRITE_TRACE=<dir> writes the file there
instead of comparing (in the manner of APE_WRITE_PINS)."""
import functools
import inspect
import json
import os

import pytest
import torch

import model_util as M
import oracle_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_trace.json")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _enc(v):
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape), "dtype": str(v.dtype), "stride": list(v.stride())}
    if isinstance(v, float):
        return {"float": repr(v)}
    if v is None or isinstance(v, (bool, int)):
        return v
    if isinstance(v, (torch.dtype, torch.device)):
        return str(v)
    if isinstance(v, (tuple, list)):
        return [_enc(x) for x in v]
    raise TypeError(f"backbone trace: argument of type {type(v).__name__}")


class Recorder:
    """wraps every public function of ape_amd.ops (after `fake_ops` put the torch definitions there): one entry per depth-0 call"""

    def __init__(self, monkeypatch):
        import ape_amd.ops as ops
        self.entries, self.depth, self.branches = [], 0, 0
        for name, fn in inspect.getmembers(ops, inspect.isfunction):
            if not name.startswith("_") and name != "fork":
                monkeypatch.setattr(ops, name, self._wrap(name, fn))
        monkeypatch.setattr(ops, "fork", self._wrap_fork(ops.fork))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*args, **kwargs):
            if self.depth == 0:
                bound = sig.bind(*args, **kwargs)
                self.entries.append({"op": name, "args": {k: _enc(v) for k, v in bound.arguments.items()}})
            self.depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self.depth -= 1
        return call

    def _wrap_fork(self, fork):
        rec = self

        class Handle:
            def __init__(self, branch, inner):
                self.branch, self.inner = branch, inner

            def join(self):
                rec.entries.append({"op": "join", "branch": self.branch})
                return self.inner.join()

        def call(fn, force=False):
            branch = self.branches
            self.branches += 1
            self.entries.append({"op": "fork", "branch": branch})          # on the CPU the closure runs inline: its ops follow here
            inner = fork(fn, force)
            self.entries.append({"op": "fork_end", "branch": branch})
            return Handle(branch, inner)
        return call

    def take(self):
        out, self.entries, self.branches = self.entries, [], 0
        return out


def _check(key, entries):
    out_dir = os.environ.get("APE_WRITE_TRACE")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "backbone_trace.json")
        done = json.load(open(path)) if os.path.exists(path) else {}
        done[key] = entries
        with open(path, "w") as f:                       # one entry per line: a changed launch is one changed line
            f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(e) for e in v) + "\n]"
                                       for k, v in sorted(done.items())) + "\n}\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)[key]
    got = json.loads(json.dumps(entries))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{key}: launch {i} differs\n  now : {json.dumps(g)}\n  pin : {json.dumps(w)}"
    assert len(got) == len(want), f"{key}: {len(got)} launches, pinned {len(want)}"


def _ti_512(dtype):
    """APE-Ti as test_host_model.test_ape_ti_backbone_matches_reference_golden builds it"""
    from ape_amd.modeling.build import build_ape
    from oracle import weights
    gold = U.load_golden("Ti_512")
    cfg_name, wseed, image, text = U.case_inputs(gold)
    model = build_ape(cfg_name)
    model.load_state_dict(weights.make_state_dict(U.load_spec(cfg_name), wseed), strict=False)
    model.model_vision.set_compute_dtype(dtype)
    return model, image


# tiny_padded: CLIP ViT-L form (rope, sub-LayerNorm, SwiGLU, pre-norm); small_E: ViT-e (post-norm, GELU, head width 112 -> 128);
# small_G: EVA-01-CLIP ViT-g (pre-norm, GELU, head width 88); small_V: vit_eva with relative positions; small_A: vit_eva02 with
# sub-LayerNorm and windows that tile the grid; Ti_512: vit_eva02 with 14 x 14 windows that do not
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["tiny_padded", "small_E", "small_G", "small_V", "small_A", "Ti_512"])
def test_backbone_launch_sequence(fake_ops, monkeypatch, case, dt):
    dtype = DTYPES[dt]
    if case == "Ti_512":
        model, image = _ti_512(dtype)
    else:
        model, image, text, gold = M.build_model(case, "cpu", dtype)
    mv = model.model_vision
    rec = Recorder(monkeypatch)
    mv.backbone.forward_tokens(image, mv._mean, mv._std)
    _check(f"{case}/{dt}", rec.take())
    if case == "tiny_padded":
        # the batched ViT pass of the benchmark's two-image step: one pass over [2 N, E], the second image of another size
        image2 = torch.randint(0, 256, (3, 256, 176), generator=torch.Generator().manual_seed(77)).float()
        mv.backbone.net.forward_tokens([image, image2], mv._mean, mv._std)
        _check(f"{case}/{dt}/two_images", rec.take())
