"""SURVEY.md section 8(f3) / VERDICT r4 item 8: the HDF5- and image-shaped entry points of discorpy_amd.losa.loadersaver
(load_hdf_file, load_hdf_object, save_hdf_file, open_hdf_stream, load_image, save_image -- reference
discorpy/losa/loadersaver.py:84-106, 248-355, 413-451, 560-656) and the stack functions fed by them.

h5py is not installed in the build image: tests/helpers/fake_h5py.py stands in for it (sys.modules["h5py"]).  Golden G20
(tools/gen_golden.py) holds what the REFERENCE's own loadersaver returned, raised and wrote on the same stand-in and the same
files, and the CPU test must match it; the GPU tests run the example_04.py call sequence -- image in, metadata file, stack from
an HDF dataset read band by band, result streamed into an HDF dataset -- against the oracle."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import HOST, ROOT, golden, noise, oblend

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fake_h5py  # noqa: E402

from discorpy_amd.losa import loadersaver as losa  # noqa: E402

@pytest.fixture
def h5(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", fake_h5py)
    return fake_h5py


def _stack_file(h5, path, dtype=">u2", shape=(9, 14, 11), key="entry/data/data"):
    vol = (np.random.default_rng(5).random(shape) * 60000).astype(dtype)
    with h5.File(path, "w") as f:
        f.create_dataset(key, data=vol)
        f.create_dataset("entry/angles", data=np.linspace(0.0, 180.0, shape[0]))
    return vol


def test_without_h5py_the_rest_of_the_module_works_and_the_hdf_entries_say_what_is_missing(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", None)            # "import h5py" raises ImportError
    p = losa.save_metadata_txt(str(tmp_path / "c.txt"), 1.5, 2.5, [1.0, 1e-3])
    assert losa.load_metadata_txt(p) == (1.5, 2.5, [1.0, 1e-3])
    (tmp_path / "x.hdf").write_text("x")
    with pytest.raises(ImportError, match="h5py"):
        losa.load_hdf_object(str(tmp_path / "x.hdf"), "entry/data")
    with pytest.raises(ImportError, match="h5py"):
        losa.open_hdf_stream(str(tmp_path / "y.hdf"), (2, 3, 4))


def test_load_hdf_file_every_index_form(h5, tmp_path):
    path = str(tmp_path / "scan.nxs")
    vol = _stack_file(h5, path)
    whole = losa.load_hdf_file(path, "entry/data/data")
    assert whole.dtype == np.float32 and np.array_equal(whole, vol.astype(np.float32))
    assert np.array_equal(losa.load_hdf_file(path), whole)                                   # key found: the first ".../data" dataset
    for axis in (0, 1, 2):
        sl = [slice(None)] * 3
        sl[axis] = 3
        one = losa.load_hdf_file(path, "entry/data/data", index=3, axis=axis)
        assert one.shape == tuple(np.delete(vol.shape, axis)) and np.array_equal(one, whole[tuple(sl)])
        sl[axis] = slice(2, 7)
        assert np.array_equal(losa.load_hdf_file(path, "entry/data/data", index=(2, 7), axis=axis), whole[tuple(sl)])
        sl[axis] = slice(1, 8, 3)
        assert np.array_equal(losa.load_hdf_file(path, "entry/data/data", index=(1, 8, 3), axis=axis), whole[tuple(sl)])
        sl[axis] = [0, 2, 5, 6]
        assert np.array_equal(losa.load_hdf_file(path, "entry/data/data", index=[0, 2, 5, 6], axis=axis), whole[tuple(sl)])
        sl[axis] = slice(4, 5)          # a range of ONE index comes back 2D -- through swapaxes, so transposed for axis 2 (as the reference)
        assert np.array_equal(losa.load_hdf_file(path, "entry/data/data", index=(4, 5), axis=axis), np.swapaxes(whole[tuple(sl)], axis, 0)[0])
    assert np.array_equal(losa.load_hdf_file(path, "entry/data/data", index=2, axis=7), whole[:, :, 2])               # axis clipped
    with pytest.raises(ValueError, match="Empty indices"):
        losa.load_hdf_file(path, "entry/data/data", index=(3, 3))
    with pytest.raises(ValueError, match="Couldn't open object with the key path: nope"):
        losa.load_hdf_file(path, "nope")
    with pytest.raises(ValueError, match="No such file"):
        losa.load_hdf_file(str(tmp_path / "absent.nxs"), "entry/data/data")
    (tmp_path / "junk.h5").write_text("not a container")
    with pytest.raises(ValueError, match="Error"):
        losa.load_hdf_file(str(tmp_path / "junk.h5"), "entry/data/data")
    # 2D datasets come back as they are; 1D / 4D are refused; a file without a ".../data" dataset needs a key
    with h5.File(str(tmp_path / "flat.h5"), "w") as f:
        f.create_dataset("entry/flat", data=np.arange(12, dtype=">i4").reshape(3, 4))
        f.create_dataset("entry/line", data=np.arange(5.0))
    flat = losa.load_hdf_file(str(tmp_path / "flat.h5"), "entry/flat")
    assert flat.shape == (3, 4) and np.array_equal(flat, np.arange(12).reshape(3, 4))
    with pytest.raises(ValueError, match="Require a 2D or 3D dataset"):
        losa.load_hdf_file(str(tmp_path / "flat.h5"), "entry/line")
    with pytest.raises(ValueError, match="Please provide the key path"):
        losa.load_hdf_file(str(tmp_path / "flat.h5"))


def test_object_stream_and_save(h5, tmp_path):
    path = str(tmp_path / "scan.hdf")
    vol = _stack_file(h5, path)
    obj = losa.load_hdf_object(path, "entry/data/data")
    assert obj.shape == vol.shape and obj.dtype == vol.dtype and obj.reads == []            # nothing read yet
    assert np.array_equal(obj[2:4, 3:9, :], vol[2:4, 3:9, :]) and len(obj.reads) == 1
    with pytest.raises(ValueError, match="Couldn't open object with the key: entry/none"):
        losa.load_hdf_object(path, "entry/none")
    # save_hdf_file: <key>/data, suffix forced, numbered copies
    out = losa.save_hdf_file(str(tmp_path / "out" / "res.dat"), vol, key_path="entry/result")
    assert str(out).endswith("res.hdf") and np.array_equal(losa.load_hdf_file(str(out), "entry/result/data"), vol.astype(np.float32))
    again = losa.save_hdf_file(str(tmp_path / "out" / "res.hdf"), vol[:2], overwrite=False)
    assert str(again).endswith("res_0000.hdf") and losa.load_hdf_file(str(again)).shape == (2,) + vol.shape[1:]
    # open_hdf_stream: an empty dataset to write into, metadata beside it
    ds = losa.open_hdf_stream(str(tmp_path / "cor" / "stack"), (4, 5, 6), key_path="entry/data", data_type="uint16",
                              options={"entry/angles": np.arange(4.0), "entry/energy": 53})
    assert ds.shape == (4, 5, 6) and ds.dtype == np.uint16 and ds.name == "/entry/data"
    ds[1:3] = 7
    back = h5.File(str(tmp_path / "cor" / "stack.hdf"), "r")
    assert np.array_equal(np.asarray(back["entry/data"])[:, 0, 0], [0, 7, 7, 0])
    assert np.array_equal(np.asarray(back["entry/angles"]), np.arange(4.0)) and int(np.asarray(back["entry/energy"])) == 53
    with pytest.raises(ValueError, match="can not be a child key-path"):
        losa.open_hdf_stream(str(tmp_path / "bad.hdf"), (2, 2, 2), key_path="entry/data", options={"entry/data/angles": [1, 2]})


def test_images_round_trip(tmp_path):
    pytest.importorskip("PIL")
    img = (noise(3, (40, 52)) * 1000.0).astype(np.float32)
    p = losa.save_image(str(tmp_path / "sub" / "a.tif"), img)
    assert np.array_equal(losa.load_image(str(p)), img)                                     # TIFF keeps float32 values
    q = losa.save_image(str(tmp_path / "a.png"), img)
    back = losa.load_image(str(q))
    assert back.dtype == np.float32 and back.min() == 0.0 and back.max() == 255.0           # anything else: stretched to uint8
    assert np.array_equal(back, np.float32(np.uint8(255.0 * (img - img.min()) / (img.max() - img.min()))))
    assert str(losa.save_image(str(tmp_path / "a.png"), img, overwrite=False)).endswith("a_0000.png")
    rgb = np.stack([np.full((8, 9), v, np.uint8) for v in (10, 20, 60)], axis=-1)
    losa.save_image(str(tmp_path / "c.png"), rgb)
    assert np.array_equal(losa.load_image(str(tmp_path / "c.png")), np.full((8, 9), 30.0, np.float32))        # channels averaged
    assert losa.load_image(str(tmp_path / "c.png"), average=False).shape == (8, 9, 3)
    with pytest.raises(ValueError, match="No such file"):
        losa.load_image(str(tmp_path / "absent.png"))
    (tmp_path / "junk.png").write_text("junk")
    with pytest.raises(ValueError):
        losa.load_image(str(tmp_path / "junk.png"))


def test_same_results_and_errors_as_the_reference_on_the_same_files(h5, tmp_path):
    """Against golden G20 (tools/gen_golden.py): what the reference's loadersaver returned, raised and wrote on the same files."""
    g = golden("g20_losa_reference")
    path = str(tmp_path / "scan.nxs")
    _stack_file(h5, path)
    calls = [dict(key_path="entry/data/data"), dict(), dict(key_path="entry/data/data", index=3), dict(key_path="entry/data/data", index=3, axis=1),
             dict(key_path="entry/data/data", index=3, axis=2), dict(key_path="entry/data/data", index=(2, 7), axis=1),
             dict(key_path="entry/data/data", index=(1, 8, 3), axis=2), dict(key_path="entry/data/data", index=[0, 2, 5, 6]),
             dict(key_path="entry/data/data", index=(4, 5), axis=1), dict(key_path="entry/data/data", index=2, axis=7)]
    for k, kw in enumerate(calls):
        want, got = g["load_%d" % k], losa.load_hdf_file(path, **kw)
        assert want.dtype == got.dtype and want.shape == got.shape and np.array_equal(want, got), kw
    for k, (kw, fn) in enumerate(((dict(key_path="nope"), "load_hdf_file"), (dict(key_path="entry/data/data", index=(3, 3)), "load_hdf_file"),
                                  (dict(key_path="entry/none"), "load_hdf_object"))):
        with pytest.raises(ValueError) as e_own:
            getattr(losa, fn)(path, **kw)
        assert str(g["err_%d" % k]) == str(e_own.value)
    # files written by one side are read by the other: the reference's file (its index and datasets, as it wrote them) is read
    # here, and the file written here holds the same index and datasets -- what the reference read back from its own file
    vol = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    a = tmp_path / "ref_out.h5"
    a.write_text(str(g["saved_index"]))
    (tmp_path / "ref_out.h5.d").mkdir()
    for key in g:
        if key.startswith("saved_") and key[6:].isdigit():
            np.save(str(tmp_path / "ref_out.h5.d" / (key[6:] + ".npy")), g[key])
    b = losa.save_hdf_file(str(tmp_path / "own_out.h5"), vol, key_path="entry/x")
    assert np.array_equal(losa.load_hdf_file(str(a)), vol) and np.array_equal(g["saved_read_back"], vol)
    assert json.load(open(str(b))) == json.loads(str(g["saved_index"]))
    for fname in sorted(os.listdir(str(b) + ".d")):
        want = g["saved_" + fname[:-4]]
        got = np.load(os.path.join(str(b) + ".d", fname))
        assert want.dtype == got.dtype and want.shape == got.shape and np.array_equal(want, got), fname
    kw = dict(key_path="entry/data", data_type="int16", options={"entry/energy": 53})
    db = losa.open_hdf_stream(str(tmp_path / "own_stream"), (2, 3, 4), **kw)
    assert db.shape == tuple(int(v) for v in g["stream_shape"]) and str(db.dtype) == str(g["stream_dtype"]) and db.name == str(g["stream_name"])
    assert sorted(f.replace("own_", "ref_", 1) for f in os.listdir(str(tmp_path)) if f.startswith("own_stream")) == [str(f) for f in g["stream_files"]]
    with pytest.raises(ValueError) as e_own:
        losa.open_hdf_stream(str(tmp_path / "o2.hdf"), (2, 2, 2), key_path="entry/data", options={"entry/data/angles": [1, 2]})
    assert str(g["err_stream"]) == str(e_own.value)
    # images: the reference's files are read here as the reference reads them, and the files written here decode (PIL) to the
    # same mode and pixels as the reference's -- so the reference reads them as it reads its own
    from PIL import Image
    img = (noise(3, (40, 52)) * 1000.0).astype(np.float32)
    for ext in ("tif", "png", "jpg"):
        pa = tmp_path / ("ref_i." + ext)
        g["img_%s_file" % ext].tofile(str(pa))
        pb = losa.save_image(str(tmp_path / ("own_i." + ext)), img)
        want = g["img_%s_load" % ext]
        assert np.array_equal(want, losa.load_image(str(pb))), ext
        assert np.array_equal(want, losa.load_image(str(pa))), ext
        with Image.open(str(pb)) as im:
            assert im.mode == str(g["img_%s_mode" % ext]) and np.array_equal(np.array(im), g["img_%s_pil" % ext]), ext


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [">u2", "<f4"])
def test_example_04_call_sequence_on_hdf_datasets(hip, orc, h5, tmp_path, dtype):
    """examples/example_04.py:60-96 with the imports swapped for discorpy_amd's (and its in-memory stack for an HDF dataset):
    image in, coefficients to a metadata file and back, a chunk of sinograms of a stack that lives in a file, the whole corrected
    stack streamed into a file -- against the oracle, the stack never read whole."""
    from discorpy_amd.losa.stream import correct_stack
    from discorpy_amd.post import postprocessing as post
    H, W, D = 240, 320, 12
    mat0 = np.round(noise(11, (H, W)) * 255.0).astype(np.float32)
    losa.save_image(str(tmp_path / "dots.tif"), mat0)
    mat0 = losa.load_image(str(tmp_path / "dots.tif"))
    xcenter, ycenter, list_fact = 160.3, 118.6, [1.0, -4e-5, 2e-7, -1e-10]
    meta = losa.save_metadata_txt(str(tmp_path / "out" / "coefficients_bw.txt"), xcenter, ycenter, list_fact)
    xcenter, ycenter, list_fact = losa.load_metadata_txt(meta)
    mat3D = np.empty((D, H, W), np.float32)
    mat3D[:] = mat0
    mat3D *= np.linspace(0.5, 1.5, D, dtype=np.float32)[:, None, None]
    mat3D = mat3D.astype(dtype)
    losa.save_hdf_file(str(tmp_path / "scan.nxs"), mat3D, key_path="entry/data")
    src = losa.load_hdf_object(str(tmp_path / "scan.nxs"), "entry/data/data")
    assert src.dtype == np.dtype(dtype) and src.reads == []
    native = mat3D.astype(np.dtype(dtype).newbyteorder("="))
    # a chunk of sinograms (the example's 14..20), read as one band of rows per depth chunk
    start_index, stop_index = 14, 20
    got = post.unwarp_chunk_slices_backward(src, xcenter, ycenter, list_fact, start_index, stop_index, blend="scipy")
    want = orc.unwarp_stack_rows(native, xcenter, ycenter, list_fact, start_index, stop_index - start_index + 1, coord_round_f32=True,
                                 poly=orc.POLY_KERNEL, blend=orc.BLEND_SCIPY)
    assert got.dtype == native.dtype and np.array_equal(got, want)
    rows_read = sum((k[1].stop - k[1].start) * (k[0].stop - k[0].start) for k in src.reads)
    assert src.reads and all(isinstance(k[1], slice) and k[1].stop - k[1].start < 40 for k in src.reads) and rows_read < D * 40
    # one sinogram (float32 result whatever the input type, postprocessing.py:224)
    one = post.unwarp_slice_backward(src, xcenter, ycenter, list_fact, 100)
    assert one.dtype == np.float32 and np.array_equal(one, orc.unwarp_slice_backward(native, xcenter, ycenter, list_fact, 100, poly=orc.POLY_KERNEL,
                                                                                    blend=oblend(orc, HOST) if dtype == "<f4" else orc.BLEND_SCIPY))
    # the whole corrected stack, streamed into a new file in passes of 64 rows
    dst = losa.open_hdf_stream(str(tmp_path / "out" / "corrected.hdf"), (D, H, W), key_path="entry/data", data_type=native.dtype.name,
                               options={"entry/xcenter": xcenter, "entry/ycenter": ycenter})
    src.reads.clear()
    passes = correct_stack(src, dst, xcenter, ycenter, list_fact, rows_per_pass=64, blend="scipy")
    assert passes == 4 and max(k[1].stop - k[1].start for k in src.reads) < 100                 # never a whole projection
    full = orc.unwarp_stack_rows(native, xcenter, ycenter, list_fact, 0, H, coord_round_f32=True, poly=orc.POLY_KERNEL, blend=orc.BLEND_SCIPY)
    assert np.array_equal(losa.load_hdf_file(str(tmp_path / "out" / "corrected.hdf"), "entry/data"), full.astype(np.float32))
