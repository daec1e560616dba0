"""The pairing tower and the Miller loop's steps of r1cs/fq12_gfx950.hpp on a real MI355X, primitive by primitive, against plain
Python (tests/fq12_tower_cases.py: the flat Fq12 of tests/bn254_pairing.py and groth16_fixtures.Fq2 / Curve).

tests/native/fq12_tower.hip (compiled here, one program per family side by side) runs one kernel per primitive in workgroups of
one wave, as the verifier's kernels, one operand record per lane over several workgroups, and returns raw Montgomery limbs: fq_half and the Fq2 helpers, the Fq6 and
Fq12 products, squares and inverses, the sparse line products, fq12_frob with k chosen per lane, cyclotomic squaring, the final
exponentiation's easy part and its program (FxProg) over slots in global memory, g2_dbl_step, g2_add_step, g2_frob1,
g2_neg_frob2 and miller_step with the kind chosen per lane.  Results are compared exactly, every coefficient must be reduced, and
the guard records behind each section must come back untouched.  The same case lists run through the host build in
tests/test_fq12_tower_host.py.

Every case runs in waves whose lanes hold one group of classes, and in waves where special and generic lanes alternate (special
at lane 0, lane 63 and every even lane).  One process under one time limit per family; after a process that did not exit with
status 0 no further family is started."""
import subprocess

import pytest

from tests import fq12_tower_cases as TC

pytestmark = pytest.mark.gpu
_state = {"failed": None}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return TC.build_device_harness(tmp_path_factory.mktemp("fq12_tower"))


@pytest.mark.parametrize("name", list(TC.FAMILIES))
def test_family_on_the_device(harness, tmp_path, name):
    if _state["failed"]:
        pytest.fail("not started: the harness process of family %r did not exit cleanly" % _state["failed"])
    sections = TC.family(name)
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    TC.write_sections(fin, sections)
    p = subprocess.run(["timeout", "-k", "10", "240", harness[name], str(fin), str(fout)], capture_output=True, text=True)
    if p.returncode != 0:
        _state["failed"] = name
        pytest.fail("harness family %r: exit status %d\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    assert p.stdout.strip() == "fq12_tower: %d sections" % len(sections)
    TC.check_outputs(fout, sections)
