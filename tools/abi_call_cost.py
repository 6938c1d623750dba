"""Host cost of marshalling one call into libln3d_hip.so, without a GPU: three entry points called with a NULL first buffer, so each
returns LN3D_ERR_BAD_ARG before anything is launched.  Arguments are built the way ln3diff_amd/ops.py builds them: plain values where
_lib declares argtypes (PROTOTYPES), ctypes wrappers per argument where it does not (the binding before the table), so the same file
measures either commit.  usage: python tools/abi_call_cost.py [calls] [repeats]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ln3diff_amd import _lib  # noqa: E402

calls = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
typed = hasattr(_lib, 'PROTOTYPES')
L = _lib.lib()
ADDR = 0x10000                                                                                   # never dereferenced
gemm_args = _lib.GemmArgs(X=None, ldx=1024, W=ADDR, ldw=1024, M=12288, N=3072, K=1024, epilogue=_lib.EPI_HEADS, out0=ADDR, out1=ADDR, out2=ADDR,
                          ldo=3072, tokens=768, tok_pad=768, heads=16, head_dim=64, transpose_mask=4)
if typed:
    def ddim_step():
        return L.ln3d_ddim_step(None, ADDR, ADDR, ADDR, 3.0, 1.1, 0.4, 0.9, 0.2, 0.0, True, 49152, 0)

    def final_layer():
        return L.ln3d_final_layer(None, ADDR, ADDR, 6144, ADDR, ADDR, ADDR, ADDR, ADDR, 16, 4, 32, 2, 1024, 0)

    def gemm():
        return L.ln3d_gemm_bf16(gemm_args, 0)
else:
    P, I64, F = C.c_void_p, C.c_int64, C.c_float

    def ddim_step():
        return L.ln3d_ddim_step(None, P(ADDR), P(ADDR), P(ADDR), F(3.0), F(1.1), F(0.4), F(0.9), F(0.2), F(0.0), int(True), I64(49152), P(0))

    def final_layer():
        return L.ln3d_final_layer(None, P(ADDR), P(ADDR), I64(6144), P(ADDR), P(ADDR), P(ADDR), P(ADDR), P(ADDR), 16, 4, 32, 2, 1024, P(0))

    def gemm():
        return L.ln3d_gemm_bf16(C.byref(gemm_args), P(0))


print("binding with %s; %d calls, %d repeats; microseconds per call" % ("argtypes" if typed else "per-argument ctypes wrappers", calls, repeats))
for fn in (ddim_step, final_layer, gemm):
    assert fn() == -1, fn.__name__                                                              # LN3D_ERR_BAD_ARG: nothing was launched
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    print("%-12s best %.3f  repeats %s" % (fn.__name__, min(us), ' '.join('%.3f' % u for u in us)))
