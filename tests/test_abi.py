"""The C-ABI library loads on a machine without a GPU, exports every entry point
include/dsp_audiorec.h declares, and rejects bad arguments on the host before any launch."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "dsp_audiorec.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:size_t|int)\s+(dsp_\w+)\s*\(", src, flags=re.M)))


@pytest.fixture(scope="module")
def lib():
    from src import _hip
    return _hip.load_library()


def test_header_declares_the_path():
    names = declared_functions()
    assert {"dsp_extract_features", "dsp_extract_lds_bytes", "dsp_knn_classify",
            "dsp_knn_workspace_bytes", "dsp_extract_general", "dsp_extract_general_workspace_bytes", "dsp_zscore_fit", "dsp_zscore_apply", "dsp_abi_version"} <= set(names)


def test_every_declared_symbol_is_exported(lib):
    from src import _hip
    for name in declared_functions():
        assert hasattr(lib, name), name
        assert name in _hip.EXPORTS, "binding does not type %s" % name


def test_abi_version(lib):
    m = re.search(r"#define DSP_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.dsp_abi_version() == int(m.group(1))


def test_lds_sizing(lib):
    assert lib.dsp_extract_lds_bytes(44100, 1102, 441) > 0
    assert lib.dsp_extract_lds_bytes(44100, 1024, 512) > 0
    assert lib.dsp_extract_lds_bytes(44100, 1102, 441) <= 80 * 1024  # two workgroups per CU
    assert 0 < lib.dsp_extract_lds_bytes(200000, 1102, 441) <= 160 * 1024  # 4.5 s: summaries only
    assert lib.dsp_extract_lds_bytes(400000, 1102, 441) == 0  # beyond one CU's LDS
    assert lib.dsp_extract_lds_bytes(0, 1102, 441) == 0
    assert lib.dsp_extract_lds_bytes(44100, 0, 441) == 0


def test_fast_layout_query(lib):
    """dsp_extract_fast_layout flips exactly where csrc/extract_layout.h (extract_fast_fits) says.

    The compile-time layout holds EXTRACT_THREADS x EXTRACT_RREG = 512 x 3 = 1536 32-sample words
    including an alignment lead of up to 7 samples, at most 128 VAD and 128 feature frames, and
    window rows of at most EXTRACT_FAST_WROW = 1280 floats:
      words  (n + 7 + 31) // 32 <= 1536            <=>  n <= 1536 * 32 - 7 = 49145
      nvcap  (n - L) // S + 1 <= 128               <=>  n <= L + 128 * S - 1
      fcap   ceil((n - L) / S) + 1 <= 128          <=>  n <= L + 127 * S
      WROW   (L + 2 * 8 + 4 + 3) & ~3 <= 1280      <=>  L + 23 <= 1283  <=>  L <= 1260
    At 1102/441 the frame limits are 1102 + 127 * 441 = 57109 > 49145, so the word count decides:
    the largest FAST max_len is 49145.  At 882/220 fcap decides: 882 + 127 * 220 = 28822 (128
    feature frames; the 129th VAD frame would only start at 882 + 128 * 220 = 29042).  The largest
    FAST frame_length is 1260 (the header's comment used to say 1256)."""
    q = lib.dsp_extract_fast_layout
    assert q(44100, 1102, 441) == 1
    assert q(66150, 1102, 441) == 0
    nmax = 1536 * 32 - 7
    assert nmax == 49145 and nmax < 1102 + 127 * 441
    assert q(nmax, 1102, 441) == 1 and q(nmax + 1, 1102, 441) == 0
    assert q(882 + 127 * 220, 882, 220) == 1 and q(882 + 127 * 220 + 1, 882, 220) == 0
    lmax = 1260
    assert ((lmax + 2 * 8 + 4 + 3) & ~3) == 1280 and ((lmax + 1 + 2 * 8 + 4 + 3) & ~3) > 1280
    assert q(44100, lmax, 441) == 1 and q(44100, lmax + 1, 441) == 0
    assert q(1, 1102, 441) == 1 and q(1, lmax + 1, 441) == 0
    # 0 wherever dsp_extract_lds_bytes is 0
    for args in ((0, 1102, 441), (44100, 0, 441), (44100, 1102, 0), (400000, 1102, 441)):
        assert lib.dsp_extract_lds_bytes(*args) == 0 and q(*args) == 0
    # the generic layout still has an on-chip plan where the compile-time one does not fit
    assert lib.dsp_extract_lds_bytes(nmax + 1, 1102, 441) > 0
    assert lib.dsp_extract_lds_bytes(44100, lmax + 1, 441) > 0


def test_host_argument_checks(lib):
    """Argument errors are returned before anything touches the device."""
    from src import _hip
    f = lib.dsp_extract_features
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    p2 = ctypes.c_void_p(p.value + 2)  # misaligned pcm
    args = lambda pcm, B, L=1102, S=441, feat=p, q=None, os_=0: (pcm, p, B, 44100, L, S, p, 1, 0.5, 0.1, 1.5,
                                                                 feat, p, p, p, os_, None, None, 0, None, 0, q, None)
    assert f(*args(p, -1)) == _hip.DSP_ERR_ARGS
    assert f(*args(p, 4, feat=None)) == _hip.DSP_ERR_ARGS
    assert f(*args(p2, 4)) == _hip.DSP_ERR_ARGS
    assert f(*args(p, 4, L=0)) == _hip.DSP_ERR_ARGS
    assert f(*args(p, 4, q=p2)) == _hip.DSP_ERR_ARGS  # misaligned clip-queue scratch
    assert f(*args(p, 4, os_=18)) == _hip.DSP_ERR_ARGS  # a result row needs DSP_OUT_ROW_WORDS words
    assert f(*args(p, 0, os_=19)) == _hip.DSP_OK
    assert f(*args(p, 0)) == _hip.DSP_OK  # empty batch: nothing to launch
    assert lib.dsp_knn_workspace_bytes(100, 100, 4097, 5) == 0
    assert lib.dsp_knn_workspace_bytes(100, 100, 33, 5) > 0  # high-dimensional screen
    assert lib.dsp_knn_workspace_bytes(100, 100, 15, 33) == 0
    assert lib.dsp_knn_workspace_bytes(100, 100, 15, 5) > 0
    k = lib.dsp_knn_classify
    assert k(p, p, 100, p, 10, 0, 3, -1, 0, p, p, p, p, 1 << 20, 0, None) == _hip.DSP_ERR_ARGS
    assert k(p, p, 100, p, 10, 15, 3, -1, 0, p, p, p, None, 0, 0, None) == _hip.DSP_ERR_WORKSPACE
    assert k(p, p, 100, p, 0, 15, 3, -1, 0, None, None, None, None, 0, 0, None) == _hip.DSP_OK
    assert lib.dsp_zscore_fit(None, 10, 15, p, p, None) == _hip.DSP_ERR_ARGS
    g = lib.dsp_extract_general
    gargs = lambda sb=2, ws=None, nws=0, n=4: (p, sb, p, None, n, 0, 44100, 1102, 441, p, 1, 0.5, 0.1, 1.5,
                                              p, p, p, p, 0, None, None, 0, None, 0, ws, nws, None)
    assert g(*gargs(sb=3)) == _hip.DSP_ERR_ARGS
    assert g(*gargs()) == _hip.DSP_ERR_WORKSPACE
    assert g(*gargs(n=0)) == _hip.DSP_OK
    one = lib.dsp_extract_general_workspace_bytes(1, 44100, 1102, 441)
    assert one > 0 and lib.dsp_extract_general_workspace_bytes(3, 44100, 1102, 441) == 3 * one
    assert lib.dsp_extract_general_workspace_bytes(1, 30 * 44100, 1102, 441) > 20 * one
    assert lib.dsp_zscore_apply(p, 0, 15, p, p, p, None) == _hip.DSP_OK


def test_no_cpu_fallback():
    """Without a HIP device the product path raises instead of computing on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from src import _hip
    from src.pipeline import FeatureExtractor, knn_classify, zscore_fit
    with pytest.raises(_hip.HipError):
        FeatureExtractor(1102, 441)
    with pytest.raises(_hip.HipError):
        knn_classify([[0.0]], [0], [[0.0]], 1)
    with pytest.raises(_hip.HipError):
        zscore_fit([[0.0]])


def test_knndiag_layout_equals_product(monkeypatch):
    """With no DSP_KNN_* override set, the diagnostic library (host code built with
    -DDSP_KNN_DIAG, the product's own device objects) lays the KNN workspace out exactly as the
    product does: seeded and unseeded matrix-core shapes, the KC = 36 pilot stride, both VALU
    screens."""
    from src import _hip
    for name in ("DSP_KNN_NSPLIT", "DSP_KNN_TARGET_WGS", "DSP_KNN_SAMPLE", "DSP_KNN_SEED", "DSP_KNN_SEED_SCALE"):
        monkeypatch.delenv(name, raising=False)
    libs = []
    for path in (_hip.LIB_PATH, os.path.join(os.path.dirname(_hip.LIB_PATH), "libdsp_audiorec_knndiag.so")):
        L = ctypes.CDLL(path)
        for fn in (L.dsp_knn_workspace_bytes, L.dsp_knn_workspace_fallbacks_offset):
            fn.restype = ctypes.c_size_t
            fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
        libs.append(L)
    for shape in [(100000, 12500, 15, 5), (100000, 100000, 15, 5), (32768, 333, 31, 25), (3000, 500, 20, 12),
                  (2000, 300, 198, 3), (8000, 1500, 16, 5)]:
        total = [L.dsp_knn_workspace_bytes(*shape) for L in libs]
        fb = [L.dsp_knn_workspace_fallbacks_offset(*shape) for L in libs]
        assert total[0] == total[1] > 0, (shape, total)
        assert fb[0] == fb[1] > 0, (shape, fb)
