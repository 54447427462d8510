"""GPU: every layer of both networks ALONE against a float64 reference (oracle/layers.py, scripts/layer_check.py).

The network tests compare logits, disparities and a handful of taps, max-normalised, against a budget of 1e-3 (1e-5 for the fp32-grade engines): a
kernel can be wrong in one halo column, one padding row of the last image or 16 of 512 output channels and stay under it, because the layers behind
it dilute the error (tests/test_layer_check_cpu.py shows seven such mistakes doing exactly that).  Here one forward runs under
SEMDEPTH_KEEP_ACTIVATIONS=1; then every layer is computed in float64 on the CPU from the GPU's OWN stored input tensor(s), with the float32 weights
that were loaded, and compared element by element with the GPU's stored output.  Upstream error never enters.  The tolerance is the per-element bound
of oracle/layers.py -- accumulation, weight planes, dropped products, output format, activation -- derived from csrc/split_fmt.hpp and not fitted.

Every op of the plan is covered, alone or inside a named composite (a conv with its fused 2x2 pool; dec/tail1 = upconv1 -> iconv1 -> disp1): the count of
uncovered ops is asserted to be zero, and the kernel families a case claims to cover are asserted from the profile labels.  The cases at frame sizes
that are no power of two also assert WHERE a kernel ran (need_at: the direct kernel on a 24-row map, the folded upconv on a 3- and a 6-row source):
the printed table carries the output maps of every kernel label.  (That no such case takes longer than the slowest 256x512 case of 8 frames is
checked by scripts/layer_check.py over its own run: seconds compare within one run only, and pytest may run a single case.)"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("layer_check", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "layer_check.py"))
LC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LC)


@pytest.fixture(scope="module", autouse=True)
def keep_activations():
    saved = os.environ.get("SEMDEPTH_KEEP_ACTIVATIONS")
    os.environ["SEMDEPTH_KEEP_ACTIVATIONS"] = "1"      # every intermediate tensor stays readable after a forward
    yield
    if saved is None:
        os.environ.pop("SEMDEPTH_KEEP_ACTIVATIONS", None)
    else:
        os.environ["SEMDEPTH_KEEP_ACTIVATIONS"] = saved


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_every_layer_alone_is_within_its_derived_bound(case):
    res = LC.run_case(case)
    for line in LC.table_lines(case, res):
        print(line)
    print(f"{LC.case_id(case)}: {len(res['rows'])} layers / composites checked in {res['seconds']:.1f} s")
    assert res["rows"]
    assert len(res["uncovered"]) == 0, ("ops of the plan that no layer check covered", res["uncovered"])
    assert not res["missing"], ("kernel families the case claims to cover did not run", res["missing"], sorted(set(res["labels"].values())))
    assert not res["unmet"], ("the case did not meet the tile edge it is there for: no", res["unmet"],
                              sorted({(label, hw) for _, label, hw in res["extents"]}))
    bad = LC.failure_lines(case, res)
    assert not bad, "\n" + "\n".join(bad)
