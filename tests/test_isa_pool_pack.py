"""CPU-only ISA check of the audio-feature calls' pool kernel (q2a_exact.hip, k_poolnorm_pack / k_poolnorm_pack5),
with tests/test_isa_loads.py's disassembly and its count: every load of a row is issued before the row's arithmetic, so
no global load may be followed at once by `s_waitcnt vmcnt(0)`. The limit is 1, not 0: the clip search loads up to 64
out_start entries and counts them with a ballot straight away, and nothing else is in flight at that point."""
import pytest

from test_isa_loads import _disasm, _pick, _serial_loads


@pytest.mark.parametrize("pattern", [r"k_poolnorm_pack5", r"k_poolnorm_packILi1E", r"k_poolnorm_packILi2E",
                                     r"k_poolnorm_packILi0E", r"k_poolnorm_packILin1E"])
def test_pool_pack_kernels_issue_their_loads_together(tmp_path, pattern):
    stats = _serial_loads(_disasm("q2a_exact.o", tmp_path))
    for k in _pick(stats, pattern):
        loads, serial = stats[k]
        assert loads >= 10, (k, loads)   # two rows and the affine operands: several 16-byte loads per lane
        assert serial <= 1, (k, loads, serial)
