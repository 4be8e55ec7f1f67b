"""tools/isa_chains.py on a hand-written listing: kernel extraction, run-length compression, resource usage (no compiler)."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

LISTING = """\t.text
_Z3fooPf: ; @_Z3fooPf
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tglobal_load_dword v1, v0, s[0:1]
\tglobal_load_dword v2, v0, s[0:1] offset:4
\ts_waitcnt vmcnt(1)
\tds_write_b32 v3, v1
\ts_waitcnt lgkmcnt(0)
\ts_barrier
.LBB0_1: ; =>This Inner Loop Header: Depth=1
\tbuffer_load_dwordx4 v[4:7], v0, s[8:11], 0 offen
\tv_mfma_f32_16x16x4_f32 a[0:3], v4, v5, a[0:3]
\tv_mfma_f32_16x16x4_f32 a[0:3], v6, v7, a[0:3]
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
\t.amdhsa_kernel _Z3fooPf
\t.end_amdhsa_kernel
.Lfunc_end0:
; Kernel info:
; TotalNumSgprs: 16
; NumVgprs: 8
; NumAgprs: 4
; TotalNumVgprs: 12
; ScratchSize: 0
; LDSByteSize: 1024 bytes/workgroup (compile time only)
; Occupancy: 8
"""


def load_tool():
    spec = importlib.util.spec_from_file_location("isa_chains", ROOT / "tools" / "isa_chains.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_chains_of_a_listing():
    tool = load_tool()
    ks = tool.kernels(LISTING)
    assert list(ks) == ["_Z3fooPf"]
    body, res = ks["_Z3fooPf"]
    assert res == {"TotalNumSgprs": 16, "NumVgprs": 8, "NumAgprs": 4, "TotalNumVgprs": 12, "ScratchSize": 0,
                   "LDSByteSize": 1024, "Occupancy": 8}
    assert tool.chains(body) == ["  global_load_dword x2", "  s_waitcnt vmcnt(1)", "  ds_write", "  s_barrier", ".LBB0_1:",
                                 "  buffer_load_dwordx4", "  v_mfma_f32_16x16x4_f32 x2", "  s_cbranch_scc1 .LBB0_1", "  s_endpgm"]
