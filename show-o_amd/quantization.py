"""Per-row symmetric int8 weight format of `Showo.set_precision(3)` (csrc/quant.hip): thin wrappers over the C ABI.

    amax = max_k |w[n,k]|;  scale[n] = amax / 127 (fp32);  q[n,k] = clamp(rint(w[n,k] / scale[n]), -127, 127)
    amax < 2^-100 (all-zero rows included): scale[n] = 1, q[n,:] = 0

Device tensors in, device tensors out.  A pre-quantised checkpoint (any positive finite scales, |q| <= 127) enters an engine through
`showo_engine_load_q8`; `set_precision(3)` itself quantises with `quantize_rows`' rule when the weights are uploaded."""
import torch

from . import _lib


def quantize_rows(w):
    """w fp32 [N, K] (GPU) -> (q int8 [N, K], scale fp32 [N]).  Raises RuntimeError when a row holds NaN or inf."""
    _lib.require_gpu()
    if w.dim() != 2:
        raise ValueError("quantize_rows takes a [N, K] matrix (rows = output features)")
    w = w.detach().float().contiguous()
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.int8, device=w.device)
    scale = torch.empty((N,), dtype=torch.float32, device=w.device)
    _lib.call("showo_quantize_rows_i8", _lib.ptr(w), N, K, _lib.ptr(q), _lib.ptr(scale), _lib.stream())
    return q, scale


def dequantize_rows(q, scale):
    """(q int8 [N, K], scale fp32 [N]) -> w fp32 [N, K] = q * scale[:, None] (one rounding)"""
    _lib.require_gpu()
    if q.dim() != 2 or q.dtype != torch.int8 or scale.shape != (q.shape[0],):
        raise ValueError("dequantize_rows takes q int8 [N, K] and scale fp32 [N]")
    q = q.contiguous()
    scale = scale.detach().float().contiguous()
    N, K = q.shape
    w = torch.empty((N, K), dtype=torch.float32, device=q.device)
    _lib.call("showo_dequantize_rows_i8", _lib.ptr(q), _lib.ptr(scale), N, K, _lib.ptr(w), _lib.stream())
    torch.cuda.current_stream().synchronize()  # q / scale may be temporaries of this call
    return w
