"""The model bank without a device: the C ABI's two new symbols, seeded construction, the member
round trip and the optimiser state of one member."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = (8, 19, 200, 2)
G = 3


def test_header_and_library_export_the_bank_symbols():
    header = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert re.search(r"int explainn_create_bank\(explainn_ctx\*\* out, int groups, int cnn_units", header)
    assert re.search(r"int explainn_groups\(const explainn_ctx\* ctx\);", header)
    from explainn_amd import _lib
    for name in ("explainn_create_bank", "explainn_groups"):
        assert name in _lib.SIGNATURES
    assert os.path.exists(_lib.LIB_PATH), "libexplainn_hip.so is not built (run build())"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("explainn_create_bank", "explainn_groups"):
        assert re.search(r" T %s$" % name, out, re.M), name


def test_seeded_construction_equals_a_sequence_of_models():
    from explainn_amd import ExplaiNN, ExplaiNNBank
    torch.manual_seed(3)
    bank = ExplaiNNBank(G, *GEOM)
    after_bank = torch.rand(1)
    torch.manual_seed(3)
    models = [ExplaiNN(*GEOM) for _ in range(G)]
    assert torch.equal(after_bank, torch.rand(1)), "the bank drew more from the generator than its members"
    for g, m in enumerate(models):
        sd = bank.member_state_dict(g)
        assert list(sd) == list(m.state_dict())
        for key, v in m.state_dict().items():
            assert sd[key].shape == v.shape and torch.equal(sd[key], v), (g, key)
    U, k, L, T = GEOM
    n = (L - k + 1) // 7
    shapes = [tuple(p.shape) for p in bank.parameters()]
    assert shapes == [(G * U, 4, k), (G * U,), (G * U,), (G * U,), (100 * G * U, n, 1), (100 * G * U,),
                      (100 * G * U,), (100 * G * U,), (G * U, 100, 1), (G * U,), (G * U,), (G * U,),
                      (G, T, U), (G, T)]
    assert [name for name, _ in bank.named_parameters()] == [name for name, _ in models[0].named_parameters()]
    assert bank.state_dict()["linears.1.num_batches_tracked"].shape == ()
    assert bank._options["n_models"] == G and bank._options["cnn_units"] == U


def test_from_models_and_member_round_trip():
    from explainn_amd import ExplaiNN, ExplaiNNBank
    torch.manual_seed(5)
    models = [ExplaiNN(*GEOM) for _ in range(G)]
    for i, m in enumerate(models):
        with torch.no_grad():
            for name, b in m.named_buffers():
                if "tracked" in name:
                    b.fill_(7)
                else:
                    b.copy_(torch.rand_like(b) + i)
    state = torch.random.get_rng_state()
    bank = ExplaiNNBank.from_models(models)
    assert torch.equal(state, torch.random.get_rng_state()), "from_models / member draw from the global generator"
    for g, m in enumerate(models):
        back = bank.member(g)
        assert type(back) is ExplaiNN and back._options == m._options
        assert list(back.state_dict()) == list(m.state_dict())
        for key, v in m.state_dict().items():
            assert torch.equal(back.state_dict()[key], v), (g, key)
    # copies, not views
    with torch.no_grad():
        bank.member(1).final.weight.add_(1.0)
    assert torch.equal(bank.member_state_dict(1)["final.weight"], models[1].final.weight)
    other = ExplaiNN(*GEOM)
    bank.load_member(2, other.state_dict())
    for key, v in other.state_dict().items():
        if "tracked" not in key:
            assert torch.equal(bank.member_state_dict(2)[key], v), key
    assert torch.equal(bank.member_state_dict(0)["linears.6.weight"], models[0].state_dict()["linears.6.weight"])
    with pytest.raises(IndexError):
        bank.member(G)
    with pytest.raises(ValueError):
        ExplaiNNBank.from_models([models[0], ExplaiNN(9, 19, 200, 2)])


def test_bank_refuses_single_model_features_without_a_device():
    from explainn_amd import ExplaiNNBank
    bank = ExplaiNNBank(2, *GEOM)
    for call in (lambda: bank.input_gradient(None, None), lambda: bank.in_silico_mutagenesis(None),
                 lambda: setattr(bank, "sync_bn", object()),
                 lambda: bank(torch.zeros(2, 4, 200, requires_grad=True))):
        with pytest.raises(ValueError, match=r"member\(g\)"):
            call()
    bank.sync_bn = None
    assert bank.sync_bn is None


def test_member_state_loads_into_a_stand_alone_optimizer():
    from explainn_amd import ExplaiNNBank, get_optimizer
    from explainn_amd.optim import member_state
    torch.manual_seed(9)
    bank = ExplaiNNBank(G, *GEOM)
    opt = torch.optim.Adam(bank.parameters(), lr=2e-3)
    for step in range(3):
        for p in bank.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    full = opt.state_dict()
    for g in range(G):
        st = member_state(opt, bank, g)
        m = bank.member(g)
        mo = get_optimizer(m.parameters(), lr=1e-3)
        mo.load_state_dict(st)
        assert mo.param_groups[0]["lr"] == 2e-3
        loaded = mo.state_dict()["state"]
        assert sorted(loaded) == list(range(14))
        for i, (name, p) in enumerate(m.named_parameters()):
            assert float(loaded[i]["step"]) == 3.0
            for key in ("exp_avg", "exp_avg_sq"):
                want = bank._member_view(name, full["state"][i][key], g)
                assert loaded[i][key].shape == p.shape and torch.equal(loaded[i][key], want), (g, name, key)


def test_bank_record_decisions():
    """Made-up loss sequences: a member that improves late, one that runs out of patience, a tie
    (no improvement, as Trainer.validate's `<`), NaN (never an improvement)."""
    from explainn_amd.selene import BankRecord
    nan, inf = float("nan"), float("inf")
    r = BankRecord(4, patience=20)
    assert r.report(10, [1.0, 1.0, 1.0, nan]) == ([0, 1, 2, 3], [0, 1, 2])
    assert r.min_loss == [1.0, 1.0, 1.0, inf] and r.best_step == [10, 10, 10, 1]
    assert r.report(20, [1.2, 1.1, 1.0, nan]) == ([0, 1, 2, 3], [])          # the tie is no improvement
    assert r.final == [False] * 4                                            # member 3: 20 < 1 + 20
    assert r.report(30, [0.9, 1.1, 1.0, nan]) == ([0, 1, 2, 3], [0])         # member 0 improves late
    assert r.final == [False, True, True, True] and not r.done()
    # final members keep stepping, but nothing of theirs is written or updated again
    assert r.report(40, [0.95, 0.1, 0.1, 0.1]) == ([0], [])
    assert r.min_loss == [0.9, 1.0, 1.0, inf] and r.best_step == [30, 10, 10, 1]
    assert r.report(50, [0.95, 0.1, 0.1, 0.1]) == ([0], [])
    assert r.final[0] and r.done()
    assert r.report(60, [0.0, 0.0, 0.0, 0.0]) == ([], [])


def test_member_files_layout_and_checkpoint_through_the_trainer(tmp_path):
    """The writers take plain tensors: file layout, columns, exactly the checkpoint keys of
    Trainer.validate, and the checkpoint resumes an existing Trainer (model, step, Adam state)."""
    from explainn_amd import ExplaiNNBank, get_loss, get_optimizer
    from explainn_amd.optim import member_state
    from explainn_amd.selene import MemberFiles, Trainer, _load_checkpoint_file
    torch.manual_seed(2)
    bank = ExplaiNNBank(G, *GEOM)
    opt = torch.optim.Adam(bank.parameters(), lr=3e-3)
    for _ in range(2):
        for p in bank.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    files = MemberFiles(str(tmp_path), G, ["aucROC", "aucPR"])
    files.train(1, 0.7)
    files.validation(1, 0.69, [0.5, 0.4])
    files.validation(1, 0.61, [0.6, 0.5])
    files.checkpoint(1, 12, bank._member_options(), bank.member_state_dict(1), 0.61, member_state(opt, bank, 1))
    for g in range(G):
        d = tmp_path / ("init.%d" % g)
        assert (d / "train.txt").read_text().splitlines()[0] == "loss"
        assert (d / "validation.txt").read_text().splitlines()[0] == "loss\taucROC\taucPR"
    assert (tmp_path / "init.1" / "train.txt").read_text() == "loss\n0.7\n"
    assert (tmp_path / "init.1" / "validation.txt").read_text().splitlines()[1:] == ["0.69\t0.5\t0.4", "0.61\t0.6\t0.5"]
    assert not (tmp_path / "init.0" / "best_model.pth.tar").exists()
    path = str(tmp_path / "init.1" / "best_model.pth.tar")
    ck = _load_checkpoint_file(path)
    assert set(ck) == {"step", "arch", "options", "state_dict", "min_loss", "optimizer"}
    assert ck["arch"] == "ExplaiNN" and ck["step"] == 12 and ck["min_loss"] == 0.61
    assert list(ck["options"]) == ["cnn_units", "kernel_size", "sequence_length", "n_features", "weights_file"]
    from explainn_amd import ExplaiNN
    o = ck["options"]
    m = ExplaiNN(o["cnn_units"], o["kernel_size"], o["sequence_length"], o["n_features"], o["weights_file"])
    tr = Trainer(m, {}, get_loss("binary"), {}, get_optimizer(m.parameters(), 1e-3),
                 output_dir=str(tmp_path / "resume"), checkpoint_resume=path, logging_verbosity=0)
    assert tr._start_step == 12 and tr._min_loss == 0.61
    for key, v in bank.member_state_dict(1).items():
        assert torch.equal(m.state_dict()[key], v), key
    st = tr.optimizer.state_dict()["state"]
    full = opt.state_dict()["state"]
    for i, (name, _) in enumerate(m.named_parameters()):
        assert float(st[i]["step"]) == 2.0
        assert torch.equal(st[i]["exp_avg_sq"], bank._member_view(name, full[i]["exp_avg_sq"], 1)), name
    assert tr.optimizer.param_groups[0]["lr"] == 3e-3


@pytest.mark.parametrize("extra", [["--filter-weights", "w.npz"], ["--sync-batchnorm"]])
def test_bank_flag_refuses_transfer_learning_and_sync_batchnorm(extra, capsys):
    from explainn_amd.train import main
    with pytest.raises(SystemExit) as e:
        main(["train.tsv", "validation.tsv", "-i", "3", "--bank"] + extra)
    assert e.value.code == 2
    assert "--bank cannot be combined with" in capsys.readouterr().err


def test_bank_options_keep_the_constructor_keys():
    from explainn_amd import ExplaiNNBank
    o = ExplaiNNBank(2, *GEOM)._options
    assert o["weights_file"] is None and o["n_models"] == 2 and o["cnn_units"] == GEOM[0]
