"""The sharded form of the multiple-choice correspondence builder (heads.visual_correspondence_dot_dataset with a communicator)
against the one-process form, on two gloo ranks with a synthetic numeric backend: same records, same marks, same generator
state at the end -- including a row whose random distractor lands on the correct pixel (the ranks agree on the first such row
and rewind together; VC_D:366).  The coordinate builder (heads.visual_correspondence_dataset) the same way: same JSON bytes,
warning lines and generator state; a vertex that fails the re-check is rewound by one process and refused by two."""
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-spatialmllm_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from mspa import heads, shard  # noqa: E402

H, W = 480, 640
N_ROWS = 60


class Backend:
    """Deterministic numbers in place of K2 / K6: sizes and projections are functions of (scene, images, position)."""

    def __init__(self, clash_row=None, clash_pixel=None, rows=None, stale_row=None):
        self.calls = []
        self.clash_row, self.clash_pixel, self.rows, self.stale_row = clash_row, clash_pixel, rows, stale_row

    def image_hw(self, scene_id):
        return (H, W)

    def common_counts(self, scene_id, pairs):
        self.calls.append(("counts", scene_id))
        if scene_id == "scene0003_00":
            return None                                        # a scene the visibility file does not know
        return [(hash_int(scene_id, a, b) % 7) * 50 for a, b in pairs]      # some rows have no common point

    def project(self, scene_id, jobs):
        self.calls.append(("project", scene_id))
        out = []
        stale = None if self.stale_row is None else self.rows[self.stale_row]
        for a, b, pos in jobs:
            ok2 = True
            if stale is not None and stale["scene_id"] == scene_id and {a, b} == {stale["image_id1"], stale["image_id2"]}:
                ok2, stale = False, None                       # a stale index: ONE vertex of that row fails the re-check
            h = hash_int(scene_id, a, b, pos)
            uv2 = (float(h % (W - 20)), float((h // 1000) % (H - 20)))
            if self.clash_row is not None:
                r = self.rows[self.clash_row]
                if r["scene_id"] == scene_id and {a, b} == {r["image_id1"], r["image_id2"]}:
                    uv2 = (float(self.clash_pixel[0]), float(self.clash_pixel[1]))
            out.append((pos * 3 + 1, (float((h // 7) % W), float((h // 11) % H)), uv2, True, ok2))
        return out


def hash_int(*parts):
    import hashlib
    return int.from_bytes(hashlib.sha256("|".join(map(str, parts)).encode()).digest()[:6], "little")


def _rows():
    rng = random.Random(3)
    rows = []
    for k in range(N_ROWS):
        s = rng.randrange(5)
        a, b = rng.sample(range(0, 400, 5), 2)
        rows.append({"scene_id": f"scene{s:04d}_00", "image_id1": f"{a:05d}", "image_id2": f"{b:05d}", "overlap": 20.0})
    return rows


def _single(clash):
    rows = _rows()
    marks = []
    rng = random.Random(9)
    be = Backend(*(clash or (None, None)), rows=rows)
    out = heads.visual_correspondence_dot_dataset(rows, be, rng=rng, on_mark=lambda *a: marks.append(a[0]))
    return out, marks, rng.getstate()


def _find_clash():
    """A row with a record and its first distractor pixel, from an unrigged run: make that row's correct pixel equal it."""
    out, _, _ = _single(None)
    live = [k for k, r in enumerate(out) if r is not None]
    k = live[len(live) // 2]
    return k, tuple(out[k]["p2_list"][1])


def _rank_main(rank, world, port, q, clash):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MSPA_DIST_BACKEND="gloo")
    ctx = shard.context_from_env(torch.device("cpu"))
    rows = _rows()
    marks = []
    rng = random.Random(9)
    be = Backend(*(clash or (None, None)), rows=rows)
    out = heads.visual_correspondence_dot_dataset(rows, be, rng=rng, on_mark=lambda *a: marks.append(a[0]), ctx=ctx)
    q.put((rank, [None if r is None else json.loads(r) for r in out], marks, rng.getstate(), sorted({s for _, s in be.calls})))
    ctx.barrier()
    ctx.close()


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_dot_dataset_two_ranks_equals_one_process_with_and_without_a_rewind():
    import torch.multiprocessing as mp
    clash_free = None
    clash = _find_clash()
    for case in (clash_free, clash):
        want, want_marks, want_state = _single(case)
        assert sum(r is not None for r in want) >= 20
        if case is not None:                                       # the rigged row really went through the rejection path
            base, _, _ = _single(None)
            assert want[case[0]] is not None and want != base
        mpc = mp.get_context("spawn")
        q = mpc.Queue()
        port = _free_port()
        procs = [mpc.Process(target=_rank_main, args=(r, 2, port, q, case)) for r in range(2)]
        for p in procs:
            p.start()
        res = {r: (out, marks, state, scenes) for r, out, marks, state, scenes in (q.get(timeout=120) for _ in procs)}
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        assert res[0][0] == json.loads(json.dumps(want))           # rank 0: every record, in row order
        assert all(r is None for r in res[1][0])
        assert sorted(res[0][1] + res[1][1]) == sorted(want_marks) and res[0][1] and res[1][1]      # every image drawn once, by its owner
        assert res[0][2] == want_state == res[1][2]                # the generator ends where one process leaves it, on every rank
        assert not (set(res[0][3]) & set(res[1][3])) and len(set(res[0][3]) | set(res[1][3])) == 5   # scenes are dealt, not shared


# ---- the coordinate head: no collective for a failed re-check, so two ranks refuse what one process rewinds --------------
def _coor_run(rows, max_points_per_pair, stale_row, ctx=None):
    warned = []
    rng = random.Random(9)
    be = Backend(rows=rows, stale_row=stale_row)
    try:
        out = heads.visual_correspondence_dataset(rows, be, rng=rng, max_points_per_pair=max_points_per_pair,
                                                  on_warn=warned.append, ctx=ctx)
    except RuntimeError as e:
        return {"raised": str(e)}
    if ctx is not None:
        assert all(r is None or isinstance(r, heads.JsonLine) for r in out)
        out = [None if r is None else bytes(r) for r in out]
    return {"out": out, "warned": warned, "state": rng.getstate(), "scenes": sorted({s for _, s in be.calls})}


def _coor_cases(rows):
    """(max_points_per_pair, stale_row): one and several points per pair, then a row (one with a record) whose first vertex
    fails the re-check."""
    out = _coor_run(rows, 2, None)["out"]
    live = [k for k, r in enumerate(out) if r is not None]
    return [(1, None), (3, None), (2, live[len(live) // 2])]


def _coor_rank_main(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MSPA_DIST_BACKEND="gloo")
    ctx = shard.context_from_env(torch.device("cpu"))
    rows = _rows()
    q.put((rank, [_coor_run(rows, mpp, stale_row, ctx) for mpp, stale_row in _coor_cases(rows)]))
    ctx.barrier()
    ctx.close()


def test_coordinate_dataset_two_ranks_equals_one_process_and_refuses_a_stale_index():
    import torch.multiprocessing as mp
    rows = _rows()
    assert len({r["scene_id"] for r in rows}) >= 3
    cases = _coor_cases(rows)
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_coor_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for n, (mpp, stale_row) in enumerate(cases):
        want = _coor_run(rows, mpp, stale_row)
        got0, got1 = res[0][n], res[1][n]
        text = "".join(want["warned"])
        assert sum(r is not None for r in want["out"]) >= 20
        assert "Visibility info not found" in text and "No common visible points" in text
        if stale_row is None:
            assert all(len(r["p1_list"]) == mpp for r in want["out"] if r is not None)
            assert got0["out"] == [None if r is None else json.dumps(r).encode() for r in want["out"]]   # rank 0: the same bytes
            assert all(r is None for r in got1["out"]) and len(got1["out"]) == len(rows)
            assert got0["state"] == want["state"] == got1["state"]     # the generator ends where one process leaves it
            assert got0["warned"] == want["warned"] and got1["warned"] == []           # the warning file is rank 0's
            assert got0["scenes"] and got1["scenes"] and not (set(got0["scenes"]) & set(got1["scenes"]))
            assert len(set(got0["scenes"]) | set(got1["scenes"])) == 5                 # scenes are dealt, not shared
        else:
            # one process: the row keeps its other point, the failed one is warned about and draws no template
            assert len(want["out"][stale_row]["p1_list"]) == mpp - 1 and text.count("is not visible in image") == 1
            assert want["state"] != _coor_run(rows, mpp, None)["state"]
            # two ranks: the owner raises the stale-index error, the other rank learns of it in the failure vote
            said = sorted((g["raised"] for g in (got0, got1)), key=lambda text: "another rank failed" in text)
            assert "failed the visibility re-check" in said[0] and "single process only" in said[0]
            assert "failed the visibility re-check" not in said[1] and "another rank failed" in said[1]


# ---- the chained build of the depth-comparison engines (draws depend on the numerics) ------------------------------------
SCENES = [f"scene{k:04d}_00" for k in range(11)]
TIED = {"scene0001_00", "scene0002_00", "scene0006_00", "scene0010_00"}       # scenes where a pair is skipped: more draws than guessed


def _fake_engine():
    for name in [m for m in sys.modules if m == "spatial_engine" or m.startswith("spatial_engine.")]:
        if not (getattr(sys.modules[name], "__file__", None) or "").startswith(PKG):     # the reference's package, imported by
            del sys.modules[name]                                                        # an earlier oracle-vs-reference test
    if sys.path[0] != PKG:
        sys.path.insert(0, PKG)
    from spatial_engine.depth_perception._coor_base import DepthCoorEngineBase

    class Info:
        def prefetched_scenes(self, ids, num_workers=8, device="cpu"):
            return iter([("resident", s) for s in ids])

        def get_sorted_keys(self):
            return list(SCENES)

    class Engine(DepthCoorEngineBase):
        CHAINED = True
        task_name = "fake_comparison"

        def __init__(self, warning_file):
            self.scene_info, self.warning_file = Info(), warning_file
            self.all_max_samples, self.max_n_points_per_image = 25, 1

        def _scene_records_on(self, scene, scene_id, _draws, dry_run=False):
            n = 3 + int(scene_id[5:9]) % 4
            draws = [random.random() for _ in range(n)]
            if dry_run:
                return []
            assert scene is None or scene == ("resident", scene_id)
            if scene_id in TIED:                                  # the evaluated scene turns out to need more of the stream
                self._warn(f"Warning: a pair of {scene_id} was skipped.\n")
                draws += [random.random(), random.random()]
            return [{"id": f"{scene_id}_{k}", "v": v, "conversations": [{"from": "human", "value": f"q{k}"}]} for k, v in enumerate(draws)]

        def generate_qa_training_single_scene(self, scene_id):
            return self._scene_records_on(None, scene_id, None)
    return Engine


def _chained_rank(rank, world, port, q, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      MSPA_DIST_BACKEND="gloo")
    ctx = shard.context_from_env(torch.device("cpu"))
    random.seed(21)
    eng = _fake_engine()(os.path.join(out_dir, f"warn_w{world}.txt"))
    eng.generate_qa_training_data(os.path.join(out_dir, f"w{world}"))
    eng.all_max_samples = 7
    eng.generate_qa_eval_data(os.path.join(out_dir, f"w{world}_val"))      # a second call in a row: the generator is in step
    q.put((rank, random.getstate()))
    ctx.barrier()
    ctx.close()


def test_chained_depth_comparison_build_equals_one_process(tmp_path):
    import torch.multiprocessing as mp
    out_dir = str(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    random.seed(21)
    eng = _fake_engine()(os.path.join(out_dir, "warn_w1.txt"))
    eng.generate_qa_training_data(os.path.join(out_dir, "w1"))
    eng.all_max_samples = 7
    eng.generate_qa_eval_data(os.path.join(out_dir, "w1_val"))
    want_state = random.getstate()
    for world in (2, 3):
        mpc = mp.get_context("spawn")
        q = mpc.Queue()
        port = _free_port()
        procs = [mpc.Process(target=_chained_rank, args=(r, world, port, q, out_dir)) for r in range(world)]
        for p in procs:
            p.start()
        states = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        assert all(s == want_state for _, s in states)
        for sub in ("", "_val"):
            a = open(os.path.join(out_dir, f"w1{sub}", "fake_comparison.jsonl"), "rb").read()
            b = open(os.path.join(out_dir, f"w{world}{sub}", "fake_comparison.jsonl"), "rb").read()
            assert a == b and len(a) > 100
        assert open(os.path.join(out_dir, "warn_w1.txt")).read() == open(os.path.join(out_dir, f"warn_w{world}.txt")).read() != ""
