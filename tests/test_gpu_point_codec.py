"""The point codec's primitives of r1cs/point_codec_gfx950.hpp on a real MI355X, primitive by primitive, against plain Python
(tests/point_codec_cases.py).

tests/native/point_codec.hip (compiled here) runs one kernel per primitive in workgroups of one wave, as the library's kernels, one
operand record per lane over several workgroups, and returns raw words: fq_sqrt (0, 1, 4, the non-residue q - 1, (q +- 1) / 2, 32
seeded residues and 32 non-residues), fq2_sqrt (zero, one, real and pure-imaginary roots, a1 alone, norms without a root, squares of
both cases of its route, 64 seeded squares), fq_is_larger and fq2_is_larger (the middle of the field from both sides, c1 deciding
before c0, values whose Montgomery form lies on the other side), and the encoders and decoders of both groups in both forms with
every refused encoding.  The guard records behind each section must come back untouched.  The same case lists run through the
host build in tests/test_point_codec_host.py.

Special and generic lanes are arranged as in tests/test_gpu_fq12_tower.py (tests/fq12_tower_cases.arrange).  One process under one
time limit per family; after a process that did not exit with status 0 no further family is started."""
import subprocess

import pytest

from tests import point_codec_cases as PC

pytestmark = pytest.mark.gpu
_state = {"failed": None}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return PC.build_device_harness(tmp_path_factory.mktemp("point_codec"))


@pytest.mark.parametrize("name", list(PC.FAMILIES))
def test_family_on_the_device(harness, tmp_path, name):
    if _state["failed"]:
        pytest.fail("not started: the harness process of family %r did not exit cleanly" % _state["failed"])
    sections = PC.family(name)
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    PC.write_sections(fin, sections)
    p = subprocess.run(["timeout", "-k", "10", "120", harness, str(fin), str(fout)], capture_output=True, text=True)
    if p.returncode != 0:
        _state["failed"] = name
        pytest.fail("harness family %r: exit status %d\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    assert p.stdout.strip() == "point_codec: %d sections" % len(sections)
    PC.check_outputs(fout, sections)
