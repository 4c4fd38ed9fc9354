"""What the GPU tests that call the bare C ABI share (tests/test_gpu_dtw_align.py, tests/test_gpu_hmm.py,
tests/crop_frame_cases.py): guarded outputs, the raw bits of float64 results, uploads, and the CSR pair
list of a list of groups (a plain helper module like tests/knn_edge_cases.py: no test, no fixture)."""
import numpy as np

GUARD = 96  # elements before and after each output


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _dev(x, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to("cuda", dtype)


class Guarded:
    """An output of ``shape`` between two guard rows of GUARD elements holding ``fill``, as is the
    output itself: what the kernel leaves untouched still holds it."""

    def __init__(self, shape, dtype, fill):
        import torch
        self.n, self.fill = int(np.prod(shape)), fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.n].view(*shape)

    def get(self):
        g = np.concatenate([self.buf[:GUARD].cpu().numpy(), self.buf[GUARD + self.n:].cpu().numpy()])
        assert (g == self.fill).all(), "a guard row was written"
        return self.view.cpu().numpy()


def csr(groups):
    start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return start, np.array([r for g in groups for r in g], np.int32)
