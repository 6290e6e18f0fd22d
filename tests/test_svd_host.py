"""CPU: the host half of the truncated SVD -- the transpose builder
(arpack_hip_csr_transpose_host: a stable counting sort, so its arrays are
SciPy's A.T.tocsr() with sorted indices, bit for bit) and svds' argument errors,
which are raised before anything touches a device."""
import numpy as np
import pytest
import scipy.sparse as sp


def _fixture_matrix(golden, name):
    g = golden(name)
    m, n = (int(v) for v in g["shape"])
    return sp.csr_matrix((g["val"], g["col"], g["rowptr"]), shape=(m, n))


def _cases(golden):
    rng = np.random.default_rng(11)
    edge = sp.random(9, 7, 0.4, random_state=rng, format="lil")
    edge[0, :] = 0.0  # an empty first and an empty last row
    edge[8, :] = 0.0
    hole = sp.random(12, 6, 0.5, random_state=rng, format="lil")
    hole[:, 3] = 0.0  # a column no row touches
    out = {"v2": _fixture_matrix(golden, "v2_tall_257"), "v3": _fixture_matrix(golden, "v3_wide_200"),
           "1x1": sp.csr_matrix(np.array([[2.5]])), "empty_first_last_row": edge.tocsr(),
           "empty_column": hole.tocsr()}
    for A in out.values():
        A.eliminate_zeros()
        A.sort_indices()
    assert np.diff(out["empty_first_last_row"].indptr)[[0, -1]].tolist() == [0, 0]
    assert 3 not in out["empty_column"].indices
    return out


@pytest.mark.parametrize("name", ["v2", "v3", "1x1", "empty_first_last_row", "empty_column"])
def test_transpose_is_scipys_bitwise(pkg, golden, name):
    A = _cases(golden)[name]
    T = A.T.tocsr()
    T.sort_indices()
    rp, col, val = pkg.csr_transpose(A.indptr, A.indices, A.data, A.shape)
    assert rp.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(rp, T.indptr.astype(np.int64))
    assert np.array_equal(col, T.indices.astype(np.int32))
    assert np.array_equal(val.view(np.int64), T.data.astype(np.float64).view(np.int64))


def test_transpose_rejects_bad_index(pkg):
    with pytest.raises(ValueError):
        pkg.csr_transpose([0, 1], [3], [1.0], (1, 3))  # column 3 of a 1 x 3 matrix
    with pytest.raises(ValueError):
        pkg.csr_transpose([0, 1], [-1], [1.0], (1, 3))


def test_svds_rejects_which(pkg, golden):
    A = _fixture_matrix(golden, "v5_small")
    with pytest.raises(ValueError):
        pkg.svds(A, k=3, which="LA")
    with pytest.raises(ValueError):
        pkg.svds(A, k=3, form="fastest")


@pytest.mark.parametrize("k", [33, 34, 70])
def test_svds_k_too_large_gives_dsaupd_code(pkg, golden, k):
    """k >= min(m, n): ncv cannot exceed k within n, dsaupd's info = -3
    (SRC/dsaupd.f: "NCV must be greater than NEV and less than or equal to N")."""
    A = _fixture_matrix(golden, "v5_small")  # 70 x 33
    with pytest.raises(pkg.ArpackError) as e:
        pkg.svds(A, k=k)
    assert e.value.info == -3
    with pytest.raises(pkg.ArpackError) as e:
        pkg.svds(A.T.tocsr(), k=k)
    assert e.value.info == -3
