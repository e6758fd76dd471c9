"""The batch path of the diffusion trainers without a device: datasets_diffusion's classes against golden g31
(tools/make_goldens_diffusion_feed.py: the reference's datasets_diffusion.py and Trainer.get_batch on the synthetic files of
tests/diffusion_feed_cases.py), EDMTrainer's loop and checkpoints on the CPU, tools/train_diffusion.py's refusals, and what the
ntm_segment_* entry points refuse before they touch a device."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import diffusion_feed_cases as C
import diffusion_train_cases as T
from ntm_amd import _lib, datasets_diffusion, diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return {which: C.write_wavs(str(tmp_path_factory.mktemp("wavs" + which)), which) for which in C.SETS}


def folder_of(folders, case):
    return folders[C.CASES[case][1]]


def driver():
    spec = importlib.util.spec_from_file_location("train_diffusion_cli", os.path.join(ROOT, "tools", "train_diffusion.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def toy_config(folder, model_dir=None, **train):
    args = diffusion.load_config("toytrajectories")
    args.dset = C.dset_args(folder, "toy")
    if model_dir is not None:
        args.model_dir = str(model_dir)
    args.train.update(train)
    return args


def host_trainer(args, folder, net=None):
    """_main's order on the CPU: the dataset seeds, the network, Adam, the loader, torch's seed from np.random, the trainer."""
    ds = C.dataset(folder, "toy")
    net = T.network() if net is None else net
    opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                           eps=args.train.optimizer.eps)
    dset = iter(torch.utils.data.DataLoader(dataset=ds, batch_size=args.train.batch, num_workers=0))
    torch.manual_seed(np.random.randint(1 << 31))
    return diffusion.EDMTrainer(args, net, opt, "cpu", backend="torch", dset=dset)


@pytest.mark.parametrize("case", list(C.CASES))
def test_picks_are_the_references(folders, case):
    ds = C.dataset(folder_of(folders, case), case)
    assert (ds.seg_len, ds.fs, ds.overfit) == (C.CASES[case][2], C.SETS[C.CASES[case][1]][0], False)
    p = ds.picks()
    got = [tuple(int(v) for v in next(p)) for _ in range(C.N_PICKS)]
    assert got == C.picks(case)


@pytest.mark.parametrize("case", list(C.CASES))
def test_host_segments_are_the_references(folders, case):
    g = C.golden()
    it = iter(C.dataset(folder_of(folders, case), case))
    segs = [next(it) for _ in range(C.N_PICKS)]
    assert all(s.dtype == np.float32 and s.shape == (C.CASES[case][2],) for s in segs)
    assert np.array_equal(np.array([np.mean(s) for s in segs], np.float32), g[f"{case}_mean"])
    assert np.array_equal(np.stack([s[:64] for s in segs]), g[f"{case}_head"])
    assert np.array_equal(np.stack([s[-64:] for s in segs]), g[f"{case}_tail"])
    assert np.array_equal(np.array([s.astype(np.float64).sum() for s in segs]), g[f"{case}_sum64"])


def test_get_batch_on_the_host_loader_gives_the_references_batches(folders):
    g = C.golden()
    tr = host_trainer(toy_config(folders["44k"]), folders["44k"])
    for i in range(C.N_BATCHES):
        x = tr.get_batch()
        assert x.shape == (C.BATCH, 512) and x.dtype == torch.float32
        T.hold(f"batch {i}", x, g["toy_batch32"][i], g["toy_batch64"][i])


def test_training_loop_reproduces_the_references_losses(folders):
    g = C.golden()
    tr = host_trainer(toy_config(folders["44k"], save_model=False), folders["44k"])
    losses = []
    tr.training_loop(max_it=2, log=lambda it, loss: losses.append(float(loss)))
    assert tr.it == 3 and len(losses) == 3
    for i, loss in enumerate(losses):
        T.hold(f"loss of iteration {i}", np.array([loss]), g["toy_loss32"][i:i + 1], g["toy_loss64"][i:i + 1])


def test_checkpoints_are_written_resumed_and_loaded_by_the_generator(folders, tmp_path):
    args = toy_config(folders["44k"], tmp_path, save_interval=2)
    tr = host_trainer(args, folders["44k"])
    tr.training_loop(max_it=4)
    files = sorted(os.listdir(tmp_path))
    assert files == ["toytrajectories-2.pt", "toytrajectories-4.pt"] and tr.it == 5
    assert tr.latest_checkpoint == f"{tmp_path}/toytrajectories-4.pt"
    # the latest id by default: `it`, the parameters and the Adam state continue
    args2 = toy_config(folders["44k"], tmp_path, save_interval=2)
    re = host_trainer(args2, folders["44k"], net=diffusion.UNet1D(args2, "cpu"))
    assert re.resume_from_checkpoint() is True and re.it == 4
    saved = torch.load(tr.latest_checkpoint, weights_only=False)
    assert saved["it"] == 4 and set(saved) == {"it", "network", "optimizer", "ema", "args"}
    for k, v in saved["network"].items():
        assert torch.equal(re.network.state_dict()[k], v), k
    for k, v in saved["ema"].items():
        assert torch.equal(re.ema.state_dict()[k], v) and torch.equal(tr.ema.state_dict()[k], v), k
    state = re.optimizer.state_dict()["state"]
    assert len(state) == len(saved["optimizer"]["state"]) > 0
    for k, st in saved["optimizer"]["state"].items():
        assert float(state[k]["step"]) == 5.0
        assert torch.equal(state[k]["exp_avg"], st["exp_avg"]) and torch.equal(state[k]["exp_avg_sq"], st["exp_avg_sq"])
    # DiffusionGenerator loads the file's "ema"
    args2.network.checkpoint = tr.latest_checkpoint
    gen = diffusion.DiffusionGenerator(args2, "cpu")
    for k, v in saved["ema"].items():
        assert torch.equal(gen.network.state_dict()[k], v), k
    re.training_loop(max_it=4)
    assert re.it == 5 and all(float(st["step"]) == 6.0 for st in re.optimizer.state_dict()["state"].values())
    # by id and by path; a path that is not there reports False and starts over
    assert re.resume_from_checkpoint(checkpoint_id=2) is True and re.it == 2
    assert re.resume_from_checkpoint(checkpoint_path=f"{tmp_path}/toytrajectories-4.pt") is True and re.it == 4
    assert re.resume_from_checkpoint(checkpoint_path=f"{tmp_path}/nothing.pt") is False and re.it == 0


def test_remove_last_checkpoint_removes_the_earlier_file(folders, tmp_path):
    args = toy_config(folders["44k"], tmp_path, save_interval=2)
    args.logging = diffusion.Config(remove_last_checkpoint=True)
    tr = host_trainer(args, folders["44k"])
    tr.training_loop(max_it=4)
    assert os.listdir(tmp_path) == ["toytrajectories-4.pt"]


def test_load_state_dict_second_attempt_is_not_strict(folders):
    tr = host_trainer(toy_config(folders["44k"]), folders["44k"])
    sd = tr.state_dict()
    key = next(iter(sd["network"]))
    partial = {"network": {k: v + 1 for k, v in sd["network"].items() if k != key}, "ema": dict(sd["ema"]), "optimizer": sd["optimizer"]}
    before = tr.network.state_dict()[key].clone()
    assert tr.load_state_dict(partial) is True
    assert torch.equal(tr.network.state_dict()[key], before)
    other = next(k for k in sd["network"] if k != key)
    assert torch.equal(tr.network.state_dict()[other], partial["network"][other])


def test_refusals(folders, tmp_path):
    cli = driver()
    with pytest.raises(NotImplementedError):
        cli.main(["--MODE", "toytrajectories"])
    with pytest.raises(NotImplementedError):
        cli.main([])
    with pytest.raises(RuntimeError, match="HIP device only"):
        cli.main(["--MODE", "toy_trajectories", "--DSET_PATH", folders["44k"], "--DEVICE", "cpu"])
    empty = tmp_path / "empty"
    empty.mkdir()
    for cls in (datasets_diffusion.TapeHissdset, datasets_diffusion.ToyTrajectories):
        with pytest.raises(AssertionError, match="empty or nonexistent folder"):
            cls(diffusion.Config(path=str(empty), fs=44100, seg_len=1024))
        ds = cls(diffusion.Config(path=folders["44k"], fs=48000, seg_len=1024))
        with pytest.raises(AssertionError, match="wrong sampling rate"):
            next(iter(ds))
    cwd = os.getcwd()
    with pytest.raises(FileNotFoundError):
        datasets_diffusion.ToyTrajectories(diffusion.Config(path=str(tmp_path / "missing"), fs=44100, seg_len=1024))
    assert os.getcwd() == cwd
    with pytest.raises(RuntimeError, match="HIP device only"):
        datasets_diffusion.DeviceSegmentFeeder(C.dataset(folders["44k"], "toy"), 4, 100, "cpu")


def test_the_driver_trains_on_the_cpu_and_resumes(folders, tmp_path, capsys):
    cli = driver()
    cfg = json.loads(json.dumps(toy_config(folders["44k"], save_interval=2)))
    import yaml
    with open(tmp_path / "conf.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    argv = ["--MODE", "toy_trajectories", "--CONFIG", str(tmp_path / "conf.yaml"), "--MODEL_DIR", str(tmp_path / "w"),
            "--BACKEND", "torch", "--OPTIMIZER", "adam", "--FEEDER", "host", "--DEVICE", "cpu"]
    tr = cli.main(argv + ["--MAX_IT", "2"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [ln["it"] for ln in lines] == [0, 1, 2] and all(np.isfinite(ln["loss"]) for ln in lines)
    assert os.listdir(tmp_path / "w") == ["toytrajectories-2.pt"] and tr.it == 3
    cfg["train"]["resume"] = True
    with open(tmp_path / "conf.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    tr = cli.main(argv + ["--MAX_IT", "3"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [ln["it"] for ln in lines] == [2, 3] and tr.it == 4


def test_the_c_entry_points_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    ok, neg, past = _lib.i64_array([0, 90]), _lib.i64_array([0, -1]), _lib.i64_array([0, 91])

    def refused(rc, name, text):
        msg = L.ntm_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and text in msg, (rc, msg)

    for name, call in (("ntm_segment_mean", lambda bank, n, st, B, ln, mean=p: L.ntm_segment_mean(bank, n, st, B, ln, mean, None)),
                       ("ntm_segment_crop", lambda bank, n, st, B, ln, mean=p: L.ntm_segment_crop(bank, n, st, mean, B, ln, p, None)),
                       ("ntm_segment_decimate",
                        lambda bank, n, st, B, ln, mean=p: L.ntm_segment_decimate(bank, n, st, mean, B, ln, p, 3, 19, 41, p, None))):
        refused(call(None, 100, ok, 2, 10), name, "null pointer")
        refused(call(p, 100, None, 2, 10), name, "null pointer")
        refused(call(p, 100, ok, 2, 10, mean=None), name, "null pointer")
        refused(call(p, 100, ok, -1, 10), name, "negative B")
        refused(call(p, 100, ok, 2, 0), name, "L must be positive")
        refused(call(p, 100, neg, 2, 10), name, "row 1 lies outside the bank")
        refused(call(p, 100, past, 2, 10), name, "row 1 lies outside the bank")
        refused(call(p, 5, ok, 1, 10), name, "row 0 lies outside the bank")
        assert call(p, 100, ok, 0, 10) == 0
    refused(L.ntm_segment_crop(p, 100, ok, p, 2, 10, None, None), "ntm_segment_crop", "null pointer")
    dec = lambda ker, orig, width, taps, out=p: L.ntm_segment_decimate(p, 100, ok, p, 2, 10, ker, orig, width, taps, out, None)   # noqa: E731
    refused(dec(None, 3, 19, 41), "ntm_segment_decimate", "null pointer")
    refused(dec(p, 3, 19, 41, out=None), "ntm_segment_decimate", "null pointer")
    refused(dec(p, 0, 19, 38), "ntm_segment_decimate", "orig must be positive")
    refused(dec(p, 3, 19, 40), "ntm_segment_decimate", "taps must be 2 width + orig")
    refused(dec(p, 3, -1, 1), "ntm_segment_decimate", "taps must be 2 width + orig")
