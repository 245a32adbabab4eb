"""The call-site rewrite a maintainer runs on the Go module (go-curdleproofs_amd/go/rewrite/rewrite_multiexp.py;
INTEGRATION.md section 2 step 3): the pattern on call shapes written here.  The count SURVEY.md section 8a gives
(39 non-test sites) needs a checkout of the module: `rewrite_multiexp.py --check DIR` verifies it there."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("rewrite_multiexp", os.path.join(ROOT, "go-curdleproofs_amd", "go", "rewrite", "rewrite_multiexp.py"))
rw = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rw)


def test_the_rule_on_the_shapes_the_module_uses():
    src = """
	if _, err := acc.MultiExp(bases, scalars, common.MultiExpConf); err != nil {
	if _, err := l.MultiExp(pkg.ToAffine(proof.Points), gammaInv, common.MultiExpConf); err != nil {
	if _, err := M.MultiExp(gs, frs, MultiExpConf); err != nil {
	res, err := other.MultiExp(a, b, ecc.MultiExpConfig{})   // another configuration: not this module's funnel
	x.MultiExpBatch(a, b, common.MultiExpConf)
"""
    out, n = rw.rewrite(src)
    assert n == 3
    assert "common.MultiExp(&acc, bases, scalars)" in out
    assert "common.MultiExp(&l, pkg.ToAffine(proof.Points), gammaInv)" in out
    assert "\tif _, err := MultiExp(&M, gs, frs); err != nil {" in out          # inside package common: unqualified
    assert "other.MultiExp(a, b, ecc.MultiExpConfig{})" in out                   # untouched
    assert "x.MultiExpBatch(a, b, common.MultiExpConf)" in out                  # a different method
    again, m = rw.rewrite(out)
    assert m == 0 and again == out                                               # idempotent
