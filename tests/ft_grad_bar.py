"""The bar a gradient of the fine-tune kernels is held to against the CPU oracle (test infrastructure, shared by
test_gpu_finetune.py::test_more_shapes_vs_cpu_oracle and test_gpu_ft_loop.py)."""
import numpy as np


# Gradients are sums of up to ~10^5 float32 terms per table row whose order is not fixed (float atomics, group-private partial
# sums): the bar is norm-wise, max |g - ref| <= 2e-5 max |ref| -- measured 6e-6 on the bs-256 batches (tools/ft_err_probe.py),
# 50x tighter than the rtol 1e-3 / atol 1e-5 this test used through round 2 -- and element-wise rtol 5e-5 where the
# reference is not itself a cancellation (|ref| > 1 % of its maximum; measured 1.4e-5)
def close(g, r, what):
    scale = max(float(np.abs(r).max()), 1e-30)
    assert float(np.abs(g - r).max()) <= 2e-5 * scale, (what, float(np.abs(g - r).max()), scale)
    sig = np.abs(r) > 0.01 * scale
    assert np.allclose(g[sig], r[sig], rtol=5e-5, atol=0.0), what
