"""The shape of the `ape_amd.evaluation` package: its public names, and how its modules reach `ape_amd.ops`.  No GPU, no build."""
import importlib
import pkgutil

import ape_amd.evaluation
from ape_amd import ops

# what `ape_amd/evaluation.py` exported when it was one file: its dir() without underscore names and imported modules
PUBLIC = ("BoundaryAPAccumulator", "COCOAccumulator", "MaskAPAccumulator", "PanopticAccumulator", "ProposalRecallAccumulator",
          "ReferringAccumulator", "SemSegAccumulator", "boundary_ap", "boundary_iou", "box_ap", "coco_eval", "coco_metrics",
          "coco_recall_points", "decode_masks", "encode_masks", "instances_to_coco_json", "mask_ap", "panoptic_quality", "proposal_recall",
          "proposal_recall_metrics", "proposal_recall_names", "proposal_recall_thresholds", "referring_metrics", "referring_scores",
          "rles_from_runs", "semantic_metrics")


def _submodules():
    names = [m.name for m in pkgutil.iter_modules(ape_amd.evaluation.__path__)]
    assert {"_common", "wire", "ap", "coco", "segmentation", "referring", "proposals"} <= set(names)
    return [importlib.import_module(f"ape_amd.evaluation.{n}") for n in names]


def test_public_names_are_importable_and_defined_in_the_package():
    for name in PUBLIC:
        obj = getattr(ape_amd.evaluation, name)
        assert callable(obj), name
        assert obj.__module__.startswith("ape_amd.evaluation."), f"{name} is defined in {obj.__module__}"


def test_modules_reach_the_kernels_through_the_ops_module_only():
    """The CPU tests replace attributes of the module `ape_amd.ops` (the `fake_ops` fixture, `monkeypatch.setattr(ops, ...)`).  That
    reaches a module only if it looks the kernel up as `ops.<name>` at call time: `from ..ops import <name>` would bind the HIP wrapper
    before the patch.  So a module that uses the kernels holds the module `ape_amd.ops` as `ops`, and none holds anything else of it."""
    with_ops = set()
    for mod in _submodules():
        if hasattr(mod, "ops"):
            assert mod.ops is ops, mod.__name__
            with_ops.add(mod.__name__.rsplit(".", 1)[1])
        for name, obj in vars(mod).items():
            if name != "ops":
                assert getattr(obj, "__module__", None) != "ape_amd.ops", f"{mod.__name__}.{name} is bound to an object of ape_amd.ops"
    assert {"wire", "ap", "coco", "segmentation", "referring", "proposals"} <= with_ops      # `_common` launches nothing
