"""Plain-torch restatement of dist2plane_matmul on the Poincare ball at k = -1 (math_.py:2125-2159 with arsinh :63-64), for any dtype,
in the reference's order of operations, and its backward written out by hand without autograd: the formulas the kernels of
csrc/dist2plane_matmul.hip evaluate, and the yardstick of tests/test_gpu_dist2plane_matmul.py.  tests/test_dist2plane_matmul_host.py
holds the forward to the reference's own recorded outputs (tests/golden/dist2plane_matmul.npz) and the hand backward to autograd.

x (..., N, D) on the ball, points p (..., D, M) on the ball, normals z (..., D, M) -> (..., N, M); i runs over the rows of x, j over the
columns of p and z:

    zn_j = |z_j|          zh_j = z_j / max(zn_j, 1e-15)
    x2_i = |x_i|^2        p2_j = |p_j|^2       bx_i = max(1 - x2_i, 1e-15)      bp_j = max(1 - p2_j, 1e-15)
    xp_ij = <x_i, p_j>    xz_ij = <x_i, zh_j>  pz_j = <p_j, zh_j>               alpha_ij = 1 - 2 xp_ij + x2_i
    t_ij  = (2 / bp_j) (xz_ij - (alpha_ij / bx_i) pz_j)                         out_ij = 2 asinh(t_ij) zn_j      (zn_j without a clamp)

asinh as the reference writes it, log(max(t + sqrt(1 + t^2), 1e-15)): below t = 0 the sum cancels, which is what makes this function
harder on fp32 than its neighbours.  It is NOT 2 dist2plane(signed, scaled) of the transposed operands (tests/dist2plane_ref.py): the
two agree only where x = 0.

Backward under the incoming gradient g; a clamp that holds passes nothing, the Euclidean norm at exactly 0 has gradient 0:

    h_ij  = 2 g_ij zn_j / sqrt(1 + t_ij^2)        C_xz = 2 h / bp_j        C_xp = 4 h pz_j / (bp_j bx_i)
    c_x2_i = sum_j -2 h pz_j / (bp_j bx_i) - 2 h alpha_ij pz_j / (bp_j bx_i^2)        (the second term 0 where bx is clamped)
    c_p2_j = sum_i h t_ij / bp_j                                                      (0 where bp is clamped)
    c_pz_j = sum_i -2 h alpha_ij / (bp_j bx_i)    c_zn_j = sum_i 2 g_ij asinh(t_ij)
    grad_x = C_xz zh^T + C_xp p^T + 2 c_x2 x      grad_p = x^T C_xp + 2 c_p2 p + c_pz zh      gzh = x^T C_xz + c_pz p
    grad_z = (gzh - zh <zh, gzh>) / zn + c_zn zh                                      (the first term 0 where zn <= 1e-15)
"""
import torch

EPS = 1e-15


def _arsinh(t):
    return (t + torch.sqrt(1 + t.pow(2))).clamp_min(EPS).log()


def _parts(x, p, z):
    zn = z.norm(dim=-2, keepdim=True, p=2)
    zh = z / zn.clamp_min(EPS)
    x2 = x.pow(2).sum(dim=-1, keepdim=True)
    p2 = p.pow(2).sum(dim=-2, keepdim=True)
    pz = (p * zh).sum(dim=-2, keepdim=True)
    alpha = 1 - 2 * torch.matmul(x, p) + x2
    t = 2 / (1 - p2).clamp_min(EPS) * (torch.matmul(x, zh) - alpha / (1 - x2).clamp_min(EPS) * pz)
    return zn, zh, x2, p2, pz, alpha, t


def dist2plane_matmul_ref(x, p, z):
    """x (..., N, D), p and z (..., D, M) -> (..., N, M)."""
    zn, _, _, _, _, _, t = _parts(x, p, z)
    return 2 * _arsinh(t) * zn


def dist2plane_matmul_bwd(x, p, z, g):
    """(grad_x, grad_p, grad_z) under the incoming gradient g (..., N, M), by the formulas above: no autograd."""
    with torch.no_grad():
        zn, zh, x2, p2, pz, alpha, t = _parts(x, p, z)
        bx, bp = (1 - x2).clamp_min(EPS), (1 - p2).clamp_min(EPS)
        bx_free, bp_free = (1 - x2 >= EPS).to(x.dtype), (1 - p2 >= EPS).to(x.dtype)
        h = 2 * g * zn / torch.sqrt(1 + t * t)
        c_xz = 2 * h / bp
        c_xp = 4 * h * pz / (bp * bx)
        c_x2 = (-2 * h * pz / (bp * bx) - bx_free * 2 * h * alpha * pz / (bp * bx * bx)).sum(dim=-1, keepdim=True)      # (..., N, 1)
        c_p2 = bp_free * (h * t / bp).sum(dim=-2, keepdim=True)                                                         # (..., 1, M)
        c_pz = (-2 * h * alpha / (bp * bx)).sum(dim=-2, keepdim=True)
        c_zn = (2 * g * torch.asinh(t)).sum(dim=-2, keepdim=True)
        xt = x.transpose(-1, -2)
        grad_x = torch.matmul(c_xz, zh.transpose(-1, -2)) + torch.matmul(c_xp, p.transpose(-1, -2)) + 2 * c_x2 * x
        grad_p = torch.matmul(xt, c_xp) + 2 * c_p2 * p + c_pz * zh
        gzh = torch.matmul(xt, c_xz) + c_pz * p
        live = zn > EPS
        through = torch.where(live, (gzh - zh * (zh * gzh).sum(dim=-2, keepdim=True)) / torch.where(live, zn, torch.ones_like(zn)),
                              torch.zeros_like(gzh))
        return grad_x, grad_p, through + c_zn * zh
