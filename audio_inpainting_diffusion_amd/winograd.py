"""The Cook-Toom construction of the Winograd forms of the 5x3 convolution, in float64 (numpy only: tools/gen_wino8.py and tools/gen_wino45.py
write csrc/aid_wino8.h and csrc/aid_wino45.h from it without loading torch; _lib's weight packs and the tests read the same matrices)."""
import numpy as np

W8_POINTS = (0.4, 0.8, 1.25, 2.5)      # F(8,3) along T: {0, +-0.4, +-0.8, +-1.25, +-2.5, inf} (tools/wino_fm3_error.py picked them)
W45_F_POINTS = (1.0, 2.0, 0.5)         # F(4,5) along the dilated row axis of the 2-D form: {0, +-1, +-2, +-1/2, inf}
W45_T_POINTS = (1.0, 2.0)              # F(4,3) along T of the 2-D form: {0, +-1, +-2, inf}


def cook_toom(points, m, r):
    """(A^T [m, n], G [n, r], B^T [n, n]) of F(m, r), n = m + r - 1, over the points {0, +-points, inf}: y = A^T [(G w) * (B^T d)].  Index order:
    0 -> point 0, 2k-1 / 2k -> +a_k / -a_k, n-1 -> infinity.  Rows of B^T are scaled to max |entry| = 1 and G by the inverse (A^T untouched);
    entries of B^T below 1e-13 are exact zeros of the construction and are stored as such."""
    n = m + r - 1
    pts = np.array([0.0] + [sg * a for a in points for sg in (1, -1)], dtype=np.float64)
    assert len(pts) == n - 1

    def vander(cols):
        V = np.zeros((n, cols))
        for j in range(n - 1):
            V[j] = pts[j] ** np.arange(cols)
        V[n - 1, cols - 1] = 1.0
        return V
    AT, G, BT = vander(m).T, vander(r), np.linalg.inv(vander(n)).T
    sc = np.abs(BT).max(axis=1)
    BT = BT / sc[:, None]
    BT[np.abs(BT) < 1e-13] = 0.0
    return AT, G * sc[:, None], BT
