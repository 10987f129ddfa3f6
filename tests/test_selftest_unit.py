"""Device run of the chain-start mixed add (add_affine_unit) through
tpst_selftest_curve's FORM_UNIT forms, on chain_start_vectors.py's edge and
random operands: the device words equal the host's (the same dispatch of
csrc/selftest_ops.h compiled with g++), equal the device's own add_affine,
and are the sums Python integers give."""
import numpy as np
import pytest

import arith_vectors as V
import chain_start_vectors as CS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    return CS.build_host_dispatch(str(tmp_path_factory.mktemp("unitg") / "test_selftest_ops"))


@pytest.mark.parametrize("form", V.LANE_FORMS)
def test_device_unit_form_equals_host(ctx, dispatch, form):
    us, p, q, unmont = CS.form_operands(form)
    dev = ctx.selftest_curve(CS.unit_op(form), p, q)
    host = CS.host_curve(dispatch, CS.unit_op(form), p, q)
    bad = np.nonzero((dev != host).any(axis=1))[0]
    assert not len(bad), (form, len(bad), us.cs.tags[bad[0]])
    full = ctx.selftest_curve(V.curve_op(form, "add_affine"), p, q)
    bad = np.nonzero((dev != full).any(axis=1))[0]
    assert not len(bad), (form, "vs add_affine", len(bad), us.cs.tags[bad[0]])
    us.check(dev, unmont, form + " unit, device")
