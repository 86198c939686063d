"""Keyword fixture of the reference's LazyConfig files for tests/test_config_kwargs.py, so that the drop-in check runs without the
reference checkout: per configuration chain, the keywords every `L(Class)(kw=...)` call passes and the attributes every
`model.model_vision[...].<kw> = ...` line assigns; and every such override of configs/**/ape_deta/*vit[lt]_eva02*.py.
Run where the reference checkout is (APE_REFERENCE, default /root/reference):  python tests/golden/make_config_kwargs.py
Writes tests/golden/config_kwargs.json (names only)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_config_kwargs as T  # noqa: E402

assert os.path.isdir(T.CFG), f"needs the reference checkout ({T.CFG})"
out = {"chains": {}, "overrides": T._live_overrides()}
for chain, files in T.CHAINS.items():
    calls, assigns = T._live_collect(files)
    out["chains"][chain] = {"calls": {k: sorted(v) for k, v in sorted(calls.items())},
                            "assigns": {k: sorted(v) for k, v in sorted(assigns.items())}}
with open(os.path.join(HERE, "config_kwargs.json"), "w") as fh:
    json.dump(out, fh, sort_keys=True)
    fh.write("\n")
