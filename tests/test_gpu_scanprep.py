"""Scan preparation on the device: the K11 kernels and the drop-in export_one_scan / batch_export against the frozen reference
outputs of tests/golden/scanprep.npz (tools/gen_scanprep_golden.py), batched launches against single-scene ones, edge sizes, the
device integer-list parser against json.loads, and the C ABI's argument checks."""
import ctypes
import hashlib
import io
import json
import os
import pickle

import numpy as np
import pytest

import scanprep_util as U
from mspa import _lib, engine, scanprep, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scanprep.npz")
SUFFIX = {"ply": "_vh_clean_2.ply", "segs": "_vh_clean_2.0.010000.segs.json", "agg": ".aggregation.json", "txt": ".txt"}


def _npy_bytes(a):
    b = io.BytesIO()
    np.save(b, a)
    return b.getvalue()


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.fixture()
def golden(tmp_path):
    g = np.load(GOLDEN)
    scans = tmp_path / "scans"
    names = [str(n) for n in g["scan_names"]]
    for name in names:
        (scans / name).mkdir(parents=True)
        for key, suffix in SUFFIX.items():
            (scans / name / (name + suffix)).write_bytes(g[f"in_{name}_{key}"].tobytes())
    (tmp_path / "labels.tsv").write_bytes(g["in_labels"].tobytes())
    (tmp_path / "names.txt").write_text("\n".join(reversed(names)) + "\n")
    return g, names, str(scans), str(tmp_path / "labels.tsv"), str(tmp_path / "names.txt")


def _check_scan_dir(g, name, d, info):
    assert _sha(os.path.join(d, "unaligned_points.npy")) == str(g[f"out_{name}_unaligned_points_sha256"])
    for f in ("aligned_points", "semantic_mask", "instance_mask"):
        assert open(os.path.join(d, f + ".npy"), "rb").read() == _npy_bytes(g[f"out_{name}_{f}"]), (name, f)
    raw = np.load(os.path.join(d, "raw_category_mask.npy"), allow_pickle=True)
    idx = g[f"out_{name}_raw_index"]
    want = np.append(g[f"out_{name}_raw_names"].astype(object), None)[idx]
    assert raw.dtype == object and raw.shape == want.shape and (raw == want).all() and all(type(x) is str for x in raw[idx >= 0][:50])
    n = g[f"out_{name}_aligned_bbox"].shape[0]
    assert info["num_objects"] == n and sorted(k for k in info if isinstance(k, int)) == list(range(n))
    assert U.same_array(info["axis_align_matrix"], g[f"out_{name}_axis_align_matrix"])
    for k in range(n):
        for w, col in (("aligned", 0), ("unaligned", 1)):
            assert U.same_array(info[k][f"{w}_bbox"], g[f"out_{name}_{w}_bbox"][k]), (name, k, w)
            assert _sha(os.path.join(d, f"object_{k}_{w}_points.npy")) == str(g[f"out_{name}_object_sha256"][k, col]), (name, k, w)
        assert info[k]["raw_category"] == str(g[f"out_{name}_object_category"][k]) and type(info[k]["raw_category"]) is str
    assert not os.path.exists(os.path.join(d, f"object_{n}_aligned_points.npy"))


@pytest.mark.gpu
def test_batch_export_writes_the_references_files(golden, tmp_path):
    BL = U.load_facade("batch_load_scannet_data")
    g, names, scans, labels, names_file = golden
    for k, device_parse in enumerate((False, True, False)):
        BL.WINDOW_ROW_WORDS = 5000 if k == 2 else 16_000_000     # third round: the membership-row bound splits the group into windows of one
        out = str(tmp_path / f"out{k}")
        BL.batch_export(None, out, names_file, labels, scans, test_mode=False, num_workers=4, device_seg_parse=device_parse)
        info = pickle.load(open(os.path.join(out, "scenes_train_val_info.pkl"), "rb"))
        assert list(info) == sorted(names)                                                        # the pickle is in sorted scan order
        for name in names:
            _check_scan_dir(g, name, os.path.join(out, name), info[name])


@pytest.mark.gpu
def test_export_one_scan_and_test_mode(golden, tmp_path):
    BL = U.load_facade("batch_load_scannet_data")
    g, names, scans, labels, names_file = golden
    name = names[1]
    got = BL.export_one_scan(name, str(tmp_path / "one"), None, labels, scans)
    _check_scan_dir(g, name, str(tmp_path / "one"), got[name])
    assert BL.worker((name, str(tmp_path / "w"), None, labels, scans, False)).keys() == {name}
    # test mode: the two point files only, an empty info dict per scan
    BL.batch_export(None, str(tmp_path / "t"), names_file, labels, scans, test_mode=True, num_workers=2)
    assert pickle.load(open(tmp_path / "t" / "scenes_test_info.pkl", "rb")) == {n: {} for n in sorted(names)}
    for n in names:
        assert sorted(os.listdir(tmp_path / "t" / n)) == ["aligned_points.npy", "unaligned_points.npy"]
        assert (tmp_path / "t" / n / "aligned_points.npy").read_bytes() == _npy_bytes(g[f"out_{n}_aligned_points"])
    # max_num_point: the same draw from the global stream, applied to the same arrays; aligned points stay whole
    np.random.seed(5)
    BL.export_one_scan(name, str(tmp_path / "m"), "1000", labels, scans)
    np.random.seed(5)
    choices = np.random.choice(g[f"out_{name}_instance_mask"].shape[0], 1000, replace=False)
    assert U.same_array(np.load(tmp_path / "m" / "instance_mask.npy"), g[f"out_{name}_instance_mask"][choices])
    assert U.same_array(np.load(tmp_path / "m" / "semantic_mask.npy"), g[f"out_{name}_semantic_mask"][choices])
    assert U.same_array(np.load(tmp_path / "m" / "unaligned_points.npy"), np.load(tmp_path / "one" / "unaligned_points.npy")[choices])
    assert (tmp_path / "m" / "aligned_points.npy").read_bytes() == _npy_bytes(g[f"out_{name}_aligned_points"])
    twelve = BL.export(**{k: v for k, v in scanprep.scan_files(scans, name).items()}, label_map_file=labels)
    assert len(twelve) == 12 and U.same_array(twelve[4], g[f"out_{name}_instance_mask"]) and U.same_array(twelve[2], g[f"out_{name}_semantic_mask"])


def _synth_scans(tmp_path, specs):
    out = []
    for k, (n, objs, align) in enumerate(specs):
        name = f"scene{k:04d}_00"
        paths = synth.write_raw_scan(str(tmp_path), name, n, objs, seed=100 + k, axis_align=align)
        files = {f: paths[f] for f in ("mesh_file", "agg_file", "seg_file", "meta_file")}
        out.append(scanprep.load_raw_scan(name, label_map=scanprep.read_label_mapping(paths["label_map_file"]), **files))
    return out


@pytest.mark.gpu
def test_one_launch_over_64_ragged_scenes_equals_64_single_launches(tmp_path):
    rng = np.random.default_rng(0)
    sizes = [1, 63, 64, 65, 1000, 4097] + rng.integers(2, 3000, 58).tolist()
    specs = [(int(n), int(rng.integers(0, 12)) if n > 40 else int(n > 1), ("z", "general", None)[k % 3]) for k, n in enumerate(sizes)]
    scans = _synth_scans(tmp_path, specs)
    dev = scanprep.default_device()
    batched = scanprep.prepare_window(scans, dev)
    assert len(batched) == 64
    for scan, b in zip(scans, batched):
        single = scanprep.prepare_window([scan], dev)[0]
        U.assert_same_export(b.as_tuple(), single.as_tuple())
        assert b.num_unique_instances == single.num_unique_instances
        want = U.numpy_export(scan)                                  # and both are the NumPy restatement the CPU tests pin to the reference
        U.assert_same_export(b.as_tuple(), want.as_tuple())
        assert b.num_unique_instances == want.num_unique_instances, scan.name


@pytest.mark.gpu
@pytest.mark.parametrize("n,objs", [(1, 1), (1, 0), (2, 1), (63, 3), (65, 3), (130, 0), (1001, 7), (4096, 5)])
def test_edge_sizes(tmp_path, n, objs):
    (scan,) = _synth_scans(tmp_path, [(n, objs, "general")])
    got = scanprep.prepare_window([scan], scanprep.default_device())[0]
    want = U.numpy_export(scan)
    U.assert_same_export(got.as_tuple(), want.as_tuple())
    assert got.num_unique_instances == want.num_unique_instances
    if objs == 0:
        assert got.unaligned_bboxes.shape == (0, 7) and got.unaligned_obj_point_clouds == [] and not got.instance_ids.any()


@pytest.mark.gpu
def test_device_int_list_parser():
    import torch
    rng = np.random.default_rng(2)
    well = [b"", b"  ", b"0", b"7", b"1,2,3", b"1, 2, 3", b" 1 ,\t2\n,\r\n3 ", b"2147483647,0", b"10,200,3000,40000,500000",
            ", ".join(map(str, rng.integers(0, 200000, 150001).tolist())).encode(), ",".join(map(str, rng.integers(0, 2 ** 31, 777).tolist())).encode()]
    values, off, status = engine.parse_int_lists_device(well, "cuda")
    host = values.cpu().numpy()
    assert status.tolist() == [0] * len(well)
    for a, text in enumerate(well):
        assert host[off[a]:off[a + 1]].tolist() == json.loads(b"[" + text + b"]"), a
    # damaged arrays between sound ones: exactly those are declined, the neighbours' values are intact
    damaged = {1: b"1,,2", 3: b"1 2", 4: b"01,5", 6: b"2147483648", 7: b"12345678901", 9: b"1,2,x", 10: b"-4,5", 12: b",1", 13: b"1,", 15: b"1.5"}
    sound = [b"5, 6, 7", b"", b"9", b"100,200", b"3", b"4,4,4,4", b"1234567890"]
    batch, k = [], 0
    for a in range(17):
        if a in damaged:
            batch.append(damaged[a])
        else:
            batch.append(sound[k % len(sound)])
            k += 1
    values, off, status = engine.parse_int_lists_device(batch, "cuda")
    host = values.cpu().numpy()
    assert [a for a in range(17) if status[a] != 0] == sorted(damaged)
    for a in range(17):
        if a not in damaged:
            assert host[off[a]:off[a + 1]].tolist() == json.loads(b"[" + batch[a] + b"]"), a
    values, off, status = engine.parse_int_lists_device([], "cuda")
    assert values.numel() == 0 and off.tolist() == [0] and status.shape == (0,)
    # expected counts: a mismatch declines; and the combined call gives the host parser's answer for every input
    assert engine.parse_int_lists_device([b"1,2,3", b"4,5"], "cuda", expected_counts=[3, 3])[2].tolist() == [0, 16]
    both = engine.parse_int_lists(batch, device="cuda")
    ref = engine.parse_int_lists(batch)
    for a in range(17):
        assert (both[a] is None) == (ref[a] is None) and (ref[a] is None or np.array_equal(both[a], ref[a])), a
    assert both[10].tolist() == [-4, 5] and both[1] is None
    torch.cuda.synchronize()


def test_c_abi_bad_arguments():
    """Validation precedes any HIP call: every new entry point answers MSPA_EINVAL to a null pointer and to a negative size."""
    lib = _lib.load()
    d = ctypes.c_void_p(64)
    E = _lib.MSPA_EINVAL
    assert lib.mspa_prep_labels(None, d, d, 1, 10, 1, d, d, d, d, d, d, d, d, None) == E and b"null pointer" in lib.mspa_last_error_string()
    assert lib.mspa_prep_labels(d, d, d, -1, 10, 1, d, d, d, d, d, d, d, d, None) == E
    assert lib.mspa_prep_labels(d, d, d, 1, 100, 1, d, d, d, d, d, d, d, d, None) == E           # 100 vertices do not fit one wave
    assert lib.mspa_prep_align(d, d, d, 1, 10, 1, None, d, None) == E
    assert lib.mspa_prep_align(d, d, d, 1, 10, 11, d, d, None) == E                              # more waves than vertices
    assert lib.mspa_prep_objects(d, d, d, d, d, 1, 10, 1, None, 1, d, 1, d, d, d, d, d, d, d, None) == E
    assert lib.mspa_prep_objects(d, d, d, d, d, 1, 10, 1, d, -1, d, 1, d, d, d, d, d, d, d, None) == E
    assert lib.mspa_prep_objects(d, d, d, d, d, 1, 10, 1, d, 1, d, 2, d, d, d, d, d, d, d, None) == E      # rows longer than the batch
    assert lib.mspa_parse_int_list_flags_device(None, d, 1, 5, d, d, None) == E
    assert lib.mspa_parse_int_list_flags_device(d, d, 1, 1 << 31, d, d, None) == E
    assert lib.mspa_parse_int_list_device(d, d, 1, 5, None, None, d, 5, d, d, None) == E
    assert lib.mspa_parse_int_list_device(d, d, 1, 5, d, None, d, -5, d, d, None) == E
    assert lib.mspa_parse_int_list_host(None, None, 1, None, None, None, None, 1) == E
    for call in (lambda: lib.mspa_prep_labels(None, None, None, 0, 0, 0, *([None] * 9)), lambda: lib.mspa_prep_align(None, None, None, 0, 0, 0, None, None, None),
                 lambda: lib.mspa_parse_int_list_device(None, None, 0, 0, None, None, None, 0, None, None, None)):
        assert call() == _lib.MSPA_OK                                                            # nothing to do
