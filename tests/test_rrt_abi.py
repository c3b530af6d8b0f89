"""The RRT entry point's parameter struct on the three sides of the ABI (no GPU): include/mpgpu.h, the ctypes
mirror and julia/MPGPU.jl's RrtParams agree field by field, and the prototype's struct name is the same type."""
import test_julia_binding as J
from motionplanning_amd import abi


def test_rrt_params_fields_agree():
    c = J.c_structs()["mp_rrt_params"]
    jl = J.jl_structs()["RrtParams"]
    assert [f for f, _, _ in c] == [f for f, _ in jl] == [f for f, _ in abi.RRTParams._fields_]
    for (f, ct, n), (_, jt) in zip(c, jl):
        assert J.jl_type_matches(jt, ct, n), (f, ct, jt)
    assert "typedef mp_rrt_params mp_rrt_params_t;" in J.header_text()


def test_rrt_ccall_passes_the_struct_by_reference():
    calls = [c for c in J.jl_ccalls() if c[0] == "mp_rrt_plan"]
    assert len(calls) == 1 and calls[0][2][1] == "Ref{RrtParams}"
    assert abi.SIGNATURES["mp_rrt_plan"][1][1] == abi.ctypes.POINTER(abi.RRTParams)
    assert len(abi.SIGNATURES["mp_rrt_plan"][1]) == len(calls[0][2]) == 20
