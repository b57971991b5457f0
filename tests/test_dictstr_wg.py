"""The dictionary-string grid (csrc/fls_dictstr.hip, FLS_DICT_WG): DICT VARCHAR
chunks decoded by one 256-thread workgroup per vector instead of by the main
decode.  Every image is decoded with the grid forced (FLS_DICT_WG=2) and
checked against the oracle, byte for byte against a decode of the same image
with the grid off (FLS_DICT_WG=0), and the FLS_DEBUG lines must show which
kernel took the string chunks."""
import struct

import numpy as np
import pytest

from helpers import assert_column_equal, gpu_decode_all

pytestmark = pytest.mark.gpu

LAUNCH = "dictstr_decode_kernel:"   # launch_dictstr's debug line
LIMIT = 64                          # kDictWgMaxEntries (fls_decode.hpp)


def _decode(fl, img, mode, monkeypatch, capfd, cols=None):
    monkeypatch.setenv("FLS_DICT_WG", str(mode))
    monkeypatch.setenv("FLS_DEBUG", "1")
    capfd.readouterr()
    t, _, out = gpu_decode_all(fl, img, cols)
    return t, out, capfd.readouterr().err


def _check_image(fl, ref, img, monkeypatch, capfd, cols=None, grid=True):
    t, new, err = _decode(fl, img, 2, monkeypatch, capfd, cols)
    assert (LAUNCH in err) == grid, err
    rf = ref.RefFile(img)
    for c, got in new.items():
        assert_column_equal(fl, rf, c, got, img.ptr)
    _, old, err0 = _decode(fl, img, 0, monkeypatch, capfd, cols)
    assert LAUNCH not in err0, err0
    for c, got in new.items():
        assert np.array_equal(got, old[c]), c
    return t, err


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 65536, 65537, 3 * 65536 + 777])
def test_row_counts(fl, ref, gpu, monkeypatch, capfd, n):
    rng = np.random.default_rng(n)
    s = [["N", "O", "DELIVER IN PERSON"][i] for i in rng.integers(0, 3, n)]
    img = fl.write_image([("s", fl.VARCHAR, s, fl.ENC_DICT)])
    _check_image(fl, ref, img, monkeypatch, capfd)


@pytest.mark.parametrize("k", [1, 2, 3, 7, LIMIT, LIMIT + 1])
def test_dictionary_sizes(fl, ref, gpu, monkeypatch, capfd, k):
    rng = np.random.default_rng(k)
    n = 3000
    words = [f"word-{i:03d}-" + "z" * (i % 9) for i in range(k)]   # <= 12 and > 12 bytes
    idx = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    img = fl.write_image([("s", fl.VARCHAR, [words[i] for i in idx], fl.ENC_DICT)])
    _, err = _check_image(fl, ref, img, monkeypatch, capfd, grid=k <= LIMIT)
    if k > LIMIT:   # a dictionary above the table limit stays on the main decode
        assert "takes 0 chunks (0 vectors), 1 DICT VARCHAR chunks stay on the main decode" in err, err


def test_inline_and_pointer_words(fl, ref, gpu, monkeypatch, capfd):
    rng = np.random.default_rng(5)
    words = ["", "a", "exactly12chr", "thirteen chars", "x" * 100]
    v = [words[i] for i in rng.integers(0, len(words), 70000)]
    img = fl.write_image([("s", fl.VARCHAR, v, fl.ENC_DICT)])
    t, _ = _check_image(fl, ref, img, monkeypatch, capfd)
    got = fl.string_t_decode(t.device_copy_out(0, 0, 5000))
    assert got == [x.encode() for x in v[:5000]]


@pytest.mark.parametrize("cols,grid", [(None, True), ([1, 2], True), ([0, 3], False)],
                         ids=["all", "with_strings", "without_strings"])
def test_mixed_table(fl, ref, gpu, monkeypatch, capfd, cols, grid):
    n = 65537
    rng = np.random.default_rng(n)
    a = rng.integers(-50, 50, n).astype(np.int32)
    b = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    s = [["N", "O", "DELIVER IN PERSON"][i] for i in rng.integers(0, 3, n)]
    img = fl.write_image([("a", fl.INT32, a, fl.ENC_FFOR), ("b", fl.INT64, b, fl.ENC_DELTA),
                          ("s", fl.VARCHAR, s, fl.ENC_DICT), ("r", fl.INT16, (b // 100).astype(np.int16), fl.ENC_RLE)])
    _check_image(fl, ref, img, monkeypatch, capfd, cols, grid)


def test_split_with_fused_fsst_launch(fl, ref, gpu, monkeypatch, capfd):
    """lineitem_full under the work-queue policy: the four DICT VARCHAR columns
    on the grid, the other main columns and l_comment's FSST chunks in the
    fused launch behind it."""
    monkeypatch.setenv("FLS_DECODE_POLICY", "64")
    monkeypatch.setenv("FLS_DICT_WG", "2")
    monkeypatch.setenv("FLS_DEBUG", "1")
    img = fl.gen_image("lineitem_full", 0.05)
    t = fl.Connection().read_image(img)
    t.device_upload()
    capfd.readouterr()
    t.device_decode()
    t.device_sync()
    err = capfd.readouterr().err
    assert LAUNCH in err and "fused_kernel" in err, err
    assert t.ncols == 16
    assert fl.check_device_table(t, "lineitem_full", 0.05) == [0] * 16


def test_out_of_range_code(fl, ref, gpu, monkeypatch, capfd):
    """A packed byte of all ones makes four codes 3 in a 3-entry dictionary:
    both paths clamp them to the last entry and report the same error."""
    words = ["aa", "b", "last"]   # inline records: the bytes do not depend on where an image copy lies
    v = [words[i % 3] for i in range(5000)]
    img = fl.write_image([("s", fl.VARCHAR, v, fl.ENC_DICT)])
    raw = bytearray(img.tobytes())
    assert struct.unpack_from("<I", raw, 256)[0] == 0x43534C46   # the first chunk's header
    packed_off = struct.unpack_from("<Q", raw, 256 + 24)[0]
    raw[256 + packed_off] = 0xFF                                 # vector 0, lane 0: values 0, 32, 64, 96
    res = {}
    for mode in (2, 0):
        monkeypatch.setenv("FLS_DICT_WG", str(mode))
        monkeypatch.setenv("FLS_DEBUG", "1")
        try:
            t = fl.Connection().read_image(bytes(raw))
        except fl.FlsError:
            pytest.skip("the reader rejects the image")
        t.device_upload()
        capfd.readouterr()
        t.device_decode()
        with pytest.raises(fl.FlsError, match="corrupt") as e:
            t.device_sync()
        assert (LAUNCH in capfd.readouterr().err) == (mode == 2)
        res[mode] = (str(e.value), t.device_copy_out(0))
    assert res[2][0] == res[0][0]
    assert np.array_equal(res[2][1], res[0][1])
    got = fl.string_t_decode(res[2][1])
    exp = [x.encode() for x in v]
    for p in (0, 32, 64, 96):
        exp[p] = b"last"
    assert got == exp
