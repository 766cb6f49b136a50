"""ctypes loader of the test-harness kernels (tests/testkit/testkit.hip -> librfuse_testkit.so, built by retrieval-fuse_amd/csrc/build.py).
Not part of the product: nothing under retrieval-fuse_amd/ loads it."""
import ctypes
from pathlib import Path

import torch  # noqa: F401  (loads libamdhip64 first)

LIB_PATH = Path(__file__).resolve().parent / 'librfuse_testkit.so'
_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError('%s not found -- build it with `python retrieval-fuse_amd/csrc/build.py`' % LIB_PATH)
        _lib = ctypes.CDLL(str(LIB_PATH))
        _lib.rft_poison_lds.argtypes = [ctypes.c_void_p]
        _lib.rft_poison_vgprs.argtypes = [ctypes.c_void_p]
        _lib.rft_f16_mfma_load.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _lib.rft_lane_reduce_probe.argtypes = [ctypes.c_void_p] * 6
        _lib.rft_block_reduce_probe.argtypes = [ctypes.c_void_p] * 7
    return _lib


def f16_mfma_load(stream, out, blocks=256, iters=60000):
    """One 154-VGPR F16-MFMA workgroup per CU (blocks = 256), ~15 ms at iters = 60000, on `stream` (a torch.cuda.Stream)."""
    assert out.numel() >= blocks * 256 and out.dtype == torch.float32
    rc = load().rft_f16_mfma_load(blocks, iters, out.data_ptr(), stream.cuda_stream)
    if rc != 0:
        raise RuntimeError('rft_f16_mfma_load: HIP error %d' % rc)


def lane_reduce_probe(din, fin):
    """One wave runs the helpers of csrc/lane_reduce.h: din [64, 18] float64 and fin [64, 8] float32 on the GPU -> (dout [64, 11], fout [64, 2], iout [64]);
    the columns are described at k_lane_reduce_probe (testkit.hip)."""
    assert din.shape == (64, 18) and din.dtype == torch.float64 and din.is_contiguous() and din.is_cuda
    assert fin.shape == (64, 8) and fin.dtype == torch.float32 and fin.is_contiguous() and fin.is_cuda
    dout = torch.empty(64, 11, dtype=torch.float64, device=din.device)
    fout = torch.empty(64, 2, dtype=torch.float32, device=din.device)
    iout = torch.empty(64, dtype=torch.int32, device=din.device)
    rc = load().rft_lane_reduce_probe(din.data_ptr(), fin.data_ptr(), dout.data_ptr(), fout.data_ptr(), iout.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError('rft_lane_reduce_probe: HIP error %d' % rc)
    return dout, fout, iout


def block_reduce_probe(din, fin, lin):
    """32 workgroups x 256 threads run the workgroup reductions of csrc/lane_reduce.h: din [32, 256, 5] float64, fin [32, 256, 2] float32 and
    lin [32, 256] int64 on the GPU -> (dout [32, 4, 5], fout [32, 3], lout [32, 2]); the rows and columns are described at k_block_reduce_probe."""
    assert din.shape == (32, 256, 5) and din.dtype == torch.float64 and din.is_contiguous() and din.is_cuda
    assert fin.shape == (32, 256, 2) and fin.dtype == torch.float32 and fin.is_contiguous() and fin.is_cuda
    assert lin.shape == (32, 256) and lin.dtype == torch.int64 and lin.is_contiguous() and lin.is_cuda
    dout = torch.empty(32, 4, 5, dtype=torch.float64, device=din.device)
    fout = torch.empty(32, 3, dtype=torch.float32, device=din.device)
    lout = torch.empty(32, 2, dtype=torch.int64, device=din.device)
    rc = load().rft_block_reduce_probe(din.data_ptr(), fin.data_ptr(), lin.data_ptr(), dout.data_ptr(), fout.data_ptr(), lout.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError('rft_block_reduce_probe: HIP error %d' % rc)
    return dout, fout, lout
