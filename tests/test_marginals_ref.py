"""CPU checks of the marginal covariances: the numpy statement (marginals_ref.py) against dense inverses, host-side
argument validation of the new C entry points (no launch), and the gtsam shim's key order and refusals."""
import ctypes

import numpy as np
import pytest

import marginals_ref as mr


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("n,band", [(13, 1), (30, 3), (45, 6), (41, 7), (50, 8), (97, 20), (77, 33), (8, 3), (17, 16)])
def test_blocked_selected_inversion_equals_dense_inverse(n, band):
    A, Sb = mr.random_spd_band(np.random.default_rng(n * 100 + band), n, band)
    assert np.array_equal(mr.band_to_dense(Sb), A)
    assert relerr(mr.selinv_band(A, band), mr.dense_to_band(np.linalg.inv(A), band)) < 1e-12


def test_stride_two_nodes_and_bias_border():
    """pose_stride 2: pose nodes 2i with padded velocity nodes 2i+1 (3 real coordinates, unit information on the padding),
    plus a shared 6-wide bias border: the band of A^-1 with the border correction is the band of the full inverse."""
    rng = np.random.default_rng(7)
    nP, band = 11, 5
    n = 2 * nP
    A, _ = mr.random_spd_band(rng, n, band)
    for i in range(nP):                     # velocity padding decoupled, unit information
        v = 6 * (2 * i + 1)
        A[v + 3:v + 6, :] = 0.0
        A[:, v + 3:v + 6] = 0.0
        A[v + 3:v + 6, v + 3:v + 6] = np.eye(3)
    Scb = 0.1 * rng.normal(size=(6 * n, 6))
    for i in range(nP):                     # the bias does not see the padding either
        Scb[6 * (2 * i + 1) + 3:6 * (2 * i + 1) + 6] = 0.0
    Sbb = np.eye(6) * 10.0 + 0.0
    Sbb += Scb.T @ np.linalg.solve(A, Scb)
    full = np.block([[A, Scb], [Scb.T, Sbb]])
    Finv = np.linalg.inv(full)
    Ainv_band = mr.band_to_dense(mr.selinv_band(A, band))
    Scc, Scb_cov, Sbb_cov = mr.border_correction(np.linalg.inv(A), Scb, Sbb)
    assert relerr(Scc, Finv[:6 * n, :6 * n]) < 1e-12
    assert relerr(Scb_cov, Finv[:6 * n, 6 * n:]) < 1e-12
    assert relerr(Sbb_cov, Finv[6 * n:, 6 * n:]) < 1e-12
    # the band of A^-1 + the rank-6 correction on the stored blocks = the band of the full inverse
    U = np.linalg.solve(A, Scb)
    corr = U @ Sbb_cov @ U.T
    ref = mr.dense_to_band(Finv[:6 * n, :6 * n], band)
    got = mr.dense_to_band(Ainv_band + corr, band)
    assert relerr(got, ref) < 1e-12
    for i in range(nP):                     # the padding coordinates keep their unit covariance
        v = 6 * (2 * i + 1)
        assert np.allclose(Finv[v + 3:v + 6, v + 3:v + 6], np.eye(3))


def test_landmark_formula_equals_dense_inverse():
    """cov_j = V_j^-1 + sum Y^T Sigma Y over pairs of observing poses, Sigma = (U - W V^-1 W^T)^-1."""
    rng = np.random.default_rng(3)
    nP, nL = 9, 14
    obs_pose, obs_point, Ws = [], [], []
    H = np.zeros((6 * nP + 3 * nL,) * 2)
    for j in range(nL):
        first = rng.integers(0, nP - 3)
        for i in range(first, first + rng.integers(1, 4)):
            J1, J2 = rng.normal(size=(3, 6)), rng.normal(size=(3, 3))
            obs_pose.append(i); obs_point.append(j); Ws.append((J1.T @ J2).reshape(-1))
            a, b = 6 * i, 6 * nP + 3 * j
            H[a:a + 6, a:a + 6] += J1.T @ J1
            H[a:a + 6, b:b + 3] += J1.T @ J2
            H[b:b + 3, a:a + 6] += J2.T @ J1
            H[b:b + 3, b:b + 3] += J2.T @ J2 + 0.1 * np.eye(3) / 3
    H[:6 * nP, :6 * nP] += np.eye(6 * nP)
    obs_pose, obs_point, W = np.array(obs_pose), np.array(obs_point), np.array(Ws)
    V = np.array([H[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3][np.triu_indices(3)] for j in range(nL)])
    Hinv = np.linalg.inv(H)
    Sig = Hinv[:6 * nP, :6 * nP]
    cov = mr.point_covariance(lambda i, k: Sig[6 * i:6 * i + 6, 6 * k:6 * k + 6], W, V, obs_pose, obs_point, nL)
    ref = np.stack([Hinv[6 * nP + 3 * j:6 * nP + 3 * j + 3, 6 * nP + 3 * j:6 * nP + 3 * j + 3] for j in range(nL)])
    assert relerr(cov, ref) < 1e-12


def _lib_or_skip():
    from visual_underwater_slam_amd import _lib
    try:
        return _lib, _lib.load()
    except OSError as e:                    # pragma: no cover - library not built
        pytest.skip(f"libvus_hip.so not loadable: {e}")


def test_new_entry_points_validate_arguments_on_the_host():
    """Every refusal happens before a launch: null pointers, band < 0, n_nodes <= 0, short work, aliasing."""
    _lib, lib = _lib_or_skip()
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: the calls below are refused on the host
    assert lib.vus_ba_band_selinv_work_doubles(0, 3) == 0
    assert lib.vus_ba_band_selinv_work_doubles(10, -1) == 0
    nw = lib.vus_ba_band_selinv_work_doubles(20, 5)
    assert nw > 0
    cases = [
        ("vus_ba_band_selinv", (None, 20, 5, fake, fake, nw, None), "null"),
        ("vus_ba_band_selinv", (fake, 0, 5, ctypes.c_void_p(0x2000), fake, nw, None), "n_nodes"),
        ("vus_ba_band_selinv", (fake, 20, -1, ctypes.c_void_p(0x2000), fake, nw, None), "band"),
        ("vus_ba_band_selinv", (fake, 20, 5, ctypes.c_void_p(0x2000), fake, nw - 1, None), "work"),
        ("vus_ba_band_selinv", (fake, 20, 5, fake, ctypes.c_void_p(0x2000), nw, None), "alias"),
        ("vus_ba_point_check", (fake, 5, None, None), "null"),
        ("vus_ba_point_check", (None, 5, fake, None), "null"),
        ("vus_ba_point_check", (fake, -1, fake, None), "n_points"),
        ("vus_ba_point_covariance", (None, fake, fake, fake, fake, 3, fake, None), "null"),
        ("vus_nav_border_covariance", (4, 2, None, fake, fake, fake, fake, fake, fake, None), "null"),
        ("vus_nav_border_covariance", (0, 2, fake, fake, fake, fake, fake, fake, fake, None), "n_nodes"),
        ("vus_nav_border_covariance", (4, -2, fake, fake, fake, fake, fake, fake, fake, None), "band"),
    ]
    for name, args, what in cases:
        rc = getattr(lib, name)(*args)
        assert rc == -1, (name, what, rc)
        assert lib.vus_last_error().decode(), (name, what)


def test_shim_joint_marginal_order_and_refusals():
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import X, L
    keys = [X(0), L(3), X(2)]
    dims = [6, 3, 6]
    full = np.arange(15 * 15, dtype=float).reshape(15, 15)
    J = gtsam.JointMarginal(sorted(keys), [dims[keys.index(k)] for k in sorted(keys)], full)
    order = sorted(keys)
    assert order == [L(3), X(0), X(2)]          # gtsam sorts keys: symbol chr 'l' < 'x'
    assert np.array_equal(J.at(L(3), X(0)), full[0:3, 3:9])
    assert np.array_equal(J.at(X(2), X(2)), full[9:15, 9:15])
    assert np.array_equal(J.fullMatrix(), full)
    assert isinstance(gtsam.KeyVector([1, 2]), list)
    assert issubclass(gtsam.IndeterminantLinearSystemException, RuntimeError)
    e = gtsam.IndeterminantLinearSystemException(L(7))
    assert "l7" in str(e) and e.key == L(7)
    with pytest.raises(NotImplementedError):
        gtsam.Marginals(gtsam.NonlinearFactorGraph(), gtsam.Values(), gtsam.Marginals.Factorization.QR)


def test_shim_names_the_key_of_a_failing_node():
    """IndeterminantSystem(kind, index) -> key: landmark index, camera node (pose 2i / velocity 2i + 1 on inertial graphs,
    pose i otherwise), the bias."""
    from visual_underwater_slam_amd import gtsam
    from visual_underwater_slam_amd.gtsam.symbol_shorthand import B, L, V, X
    mg = object.__new__(gtsam.Marginals)
    mg._pose_keys, mg._vel_keys, mg._lm_keys, mg._bias_key = [X(0), X(1), X(2)], [V(0), V(1), V(2)], [L(4), L(9)], B(0)
    assert mg._key_of("point", 1) == L(9)
    assert mg._key_of("node", 4) == X(2) and mg._key_of("node", 3) == V(1)
    assert mg._key_of("bias", 0) == B(0)
    mg._vel_keys, mg._bias_key = [], None
    assert mg._key_of("node", 2) == X(2)
