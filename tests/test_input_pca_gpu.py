"""GPU: freud_amd.input_pca end to end on a tiny shard directory (d = 40, 6 files x 70 frames): the scatter within the derived bound
of tests/input_cov_reference.py for every form of the centre, with and without lengths; the eigenvalues within Weyl's bound plus the
solver's own error; the PCA curve of planted rank-3 data; the frame count of the moments; the caller's RNG; the command line."""
import json

import numpy as np
import pytest
import torch

from tests import input_cov_reference as R

pytestmark = pytest.mark.gpu
FILES, T, D = 6, 70, 40
LENGTHS = [70, 1, 33, 99, 69, 2]
GIVEN = np.linspace(-3.0, 3.0, D)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from freud_amd.loader import write_shards
    rng = np.random.default_rng(21)
    x = rng.standard_normal((FILES, T, D)) * np.linspace(2.0, 0.2, D)
    x[:, :, 7] += 800.0
    x = x.astype(np.float32)
    folder = str(tmp_path_factory.mktemp("pca") / "shards")
    write_shards(folder, "enc", x.reshape(FILES, T * D), [T, D])
    return folder, x


@pytest.mark.parametrize("with_lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("center", ["mean", "zero", "given"])
def test_input_covariance_within_the_bound_and_weyl(shards, center, with_lengths):
    from freud_amd.input_pca import input_covariance
    from freud_amd.input_stats import input_statistics
    folder, x = shards
    lengths = LENGTHS if with_lengths else None
    torch.manual_seed(5)
    before = torch.get_rng_state()
    ic = input_covariance(folder, "enc", lengths=lengths, center=GIVEN if center == "given" else center)
    assert torch.equal(torch.get_rng_state(), before)
    st = input_statistics(folder, "enc", lengths=lengths, iterations=1)
    N = sum(R.counts(FILES, T, lengths))
    assert (ic.n_files, ic.n_frames, ic.d) == (FILES, N, D) and ic.n_frames == st.n_frames
    assert ic.mean.tobytes() == st.mean.tobytes()
    want_center = {"mean": st.mean, "zero": np.zeros(D), "given": GIVEN}[center]
    assert ic.center.dtype == np.float64 and np.array_equal(ic.center, want_center) and ic.centered_on_mean == (center == "mean")
    assert ic.summary()["center"] == center
    ref = R.reference(R.operands(x, lengths, ic.center))
    bad = R.check(ic.scatter, x, lengths, ic.center, ref=ref)
    assert bad == [], bad
    # Weyl, plus the solver's error on either side
    S_ref = np.asarray(ref[0], np.float64)
    lam_ref = np.linalg.eigvalsh(S_ref)[::-1]
    tol = float(np.linalg.norm(ic.scatter - S_ref)) + R.u64 * float(np.linalg.norm(S_ref)) + R.solver_error(ic.scatter) + R.solver_error(S_ref)
    assert np.all(np.abs(ic.eigenvalues - np.maximum(lam_ref, 0.0)) <= tol)
    assert ic.pca_fvu(0) == 1.0 and ic.pca_fvu(D) <= D * tol / np.trace(S_ref)
    if center == "mean":
        # the denominator is the one of the input statistics over the same frames: N total_variance
        assert np.trace(ic.scatter) == pytest.approx(st.total_variance * N, rel=1e-12)


def test_planted_rank_three_data_drops_to_the_noise_share(tmp_path):
    from freud_amd.input_pca import input_covariance
    from freud_amd.loader import write_shards
    x = R.planted_sample(FILES, T, D, rank=3, noise=1e-2)
    folder = str(tmp_path / "planted")
    write_shards(folder, "enc", x.reshape(FILES, T * D), [T, D])
    ic = input_covariance(folder, "enc", center="mean")
    ref = R.reference(R.operands(x, None, ic.center))
    S_ref = np.asarray(ref[0], np.float64)
    lam = np.maximum(np.linalg.eigvalsh(S_ref)[::-1], 0.0)
    tol = float(np.linalg.norm(ic.scatter - S_ref)) + R.u64 * float(np.linalg.norm(S_ref)) + R.solver_error(ic.scatter) + R.solver_error(S_ref)
    trace = float(np.trace(S_ref))
    for r in (0, 1, 2, 3, 4, D):
        want = 1.0 - lam[:r].sum() / trace
        assert abs(ic.pca_fvu(r) - want) <= (r + D) * tol / (trace - D * tol) + 4 * D * R.u64, r
    # the planted shares: the noise holds d sigma^2 of the variance, three directions 9 + 4 + 2.25
    noise_share = D * 1e-4 / (15.25 + D * 1e-4)
    assert ic.pca_fvu(2) > 0.1 and 0.5 * noise_share < ic.pca_fvu(3) < noise_share * 1.2
    assert ic.rank_for_fvu(1e-3) == 3 and 2.0 < ic.participation_ratio < 3.0
    # the held-out form on the same kind of data about this sample's centre
    y = R.planted_sample(FILES, T, D, rank=3, noise=1e-2, seed=4)[:3]
    other = str(tmp_path / "other")
    write_shards(other, "enc", y.reshape(3, T * D), [T, D])
    held = input_covariance(other, "enc", center=ic.center)
    assert abs(ic.heldout_fvu(held, 3) - held.pca_fvu(3)) < noise_share
    with pytest.raises(ValueError, match="about THIS sample's centre"):
        ic.heldout_fvu(input_covariance(other, "enc", center="zero"), 3)


def test_sample_covariance_matches_the_front_door(shards):
    from freud_amd.input_pca import input_covariance, sample_covariance
    folder, x = shards
    dev = torch.from_numpy(x).cuda()
    lens = torch.tensor([min(l, T) for l in LENGTHS], dtype=torch.int32, device="cuda")
    moments, cen, scatter = sample_covariance(dev, lens, "mean")
    ic = input_covariance(folder, "enc", lengths=LENGTHS)
    assert scatter.tobytes() == ic.scatter.tobytes() and cen.tobytes() == ic.center.tobytes() == moments[:D].tobytes()
    assert int(moments[4 * D + 1]) == ic.n_frames
    # fewer files than the directory holds
    assert input_covariance(folder, "enc", files=2).n_frames == 2 * T


def test_command_line(shards, tmp_path, capsys):
    from freud_amd.input_pca import InputCovariance, input_covariance, main
    folder, _x = shards
    lengths = str(tmp_path / "lengths.npy")
    np.save(lengths, np.array(LENGTHS))
    out = str(tmp_path / "cov.npz")
    main(["--data-path", folder, "--layer-name", "enc", "--files", "6", "--lengths", lengths, "--center", "zero", "--out", out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    ic = input_covariance(folder, "enc", lengths=LENGTHS, center="zero")
    assert line["out"] == out and line["n_frames"] == ic.n_frames and line["center"] == "zero" and "not comparable" in line["fvu_about"]
    assert line["pca_fvu"] == {"8": ic.pca_fvu(8), "16": ic.pca_fvu(16), "32": ic.pca_fvu(32)}
    assert InputCovariance.load(out) == ic
    main(["--data_path", folder, "--layer_name", "enc"])                   # no --out: the summary alone, about the mean
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["out"] is None and line["center"] == "mean"
