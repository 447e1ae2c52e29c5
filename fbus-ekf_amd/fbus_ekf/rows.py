"""Ready-made sensors for the general linearised measurement update (BatchedFilter.correct_rows, fbus_ekf_correct_rows in
include/fbus_ekf.h): plain torch functions that turn the current state and a reading into the innovation and the Jacobian rows.

Each takes nominal (B, 19) -- p v q ba bg g -- and rot (B, 9), the CARRIED rotation (row-major, the one every built-in update
linearises with), as BatchedFilter.get_state_dev() returns them, on any device (the CPU included), float32 or float64, and returns
    res (B, m) = z - h(x)        H (B, m, nstate), columns in the error-state order p v theta ba bg [g]
in the dtype and on the device of `nominal`.  The rotation error follows the injection, q <- q (x) dq(dtheta), i.e.
R_true ~ R (I + [dtheta]x).  Nothing here synchronises or leaves the device; the loop of a sensor between camera frames is

    f.predict_n(acc, gyr, dt)                                   # the IMU samples since the last reading
    nominal, rot = f.get_state_dev()[:2]                        # the linearisation point, on the device
    res, H = rows.position_fix(nominal, rot, z, lever)          # 20 lines of torch per sensor
    f.correct_rows(res, H, var)                                 # gain, injection, covariance, NIS, gate, likelihood

A sensor of one's own is written the same way: h and its derivative along p (additive) and theta (R <- R exp([dtheta]x))."""
import torch


def _vec(x, like, n=3):
    """x as a (n,) or (B, n) tensor of like's dtype and device"""
    return torch.as_tensor(x, dtype=like.dtype, device=like.device).reshape(-1, n) if x is not None else None


def _skew(v):
    """(B, 3) -> (B, 3, 3), [v]x"""
    z = torch.zeros_like(v[:, 0])
    return torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], dim=1).reshape(-1, 3, 3)


def _parts(nominal, rot, nstate):
    if nstate not in (18, 15):
        raise ValueError(f"nstate must be 18 or 15, got {nstate}")
    if nominal.ndim != 2 or nominal.shape[1] != 19 or rot.numel() != 9 * nominal.shape[0]:
        raise ValueError(f"nominal must be (B, 19) and rot (B, 9), got {tuple(nominal.shape)} and {tuple(rot.shape)}")
    return nominal[:, 0:3], rot.reshape(-1, 3, 3).to(nominal.dtype)


def position_fix(nominal, rot, z, lever=None, nstate=18):
    """An acoustic fix (USBL / LBL) of the transponder's world position, three rows.  lever: the transponder's position in the IMU
    frame, (3,) or (B, 3); None = 0.
        h(x) = p + R lever        H_p = I (columns 0..2)        H_theta = -R [lever]x (columns 6..8)        every other column 0
    z: (B, 3).  Returns res (B, 3), H (B, 3, nstate)."""
    p, R = _parts(nominal, rot, nstate)
    B = p.shape[0]
    H = torch.zeros(B, 3, nstate, dtype=p.dtype, device=p.device)
    H[:, :, 0:3] = torch.eye(3, dtype=p.dtype, device=p.device)
    h = p
    if lever is not None:
        lv = _vec(lever, p).expand(B, 3)
        h = p + torch.einsum("bij,bj->bi", R, lv)
        H[:, :, 6:9] = -R @ _skew(lv)
    return _vec(z, p) - h, H


def direction(nominal, rot, z, world_vec, mount=None, nstate=18):
    """A known world-frame vector seen in the instrument frame -- a magnetometer with the local field, a compass -- three rows.
    world_vec: the vector m_w in the world frame, (3,) or (B, 3); mount: the rotation C from the IMU frame to the instrument frame,
    (3, 3) row-major; None = the identity.
        h(x) = C R' m_w        H_theta = C [R' m_w]x (columns 6..8)        every other column 0
    z: (B, 3), the vector as the instrument reads it.  Returns res (B, 3), H (B, 3, nstate).  (No Euler angle anywhere: no singularity.)"""
    p, R = _parts(nominal, rot, nstate)
    B = p.shape[0]
    y = torch.einsum("bji,bj->bi", R, _vec(world_vec, p).expand(B, 3))          # R' m_w
    S = _skew(y)
    h = y
    if mount is not None:
        C = torch.as_tensor(mount, dtype=p.dtype, device=p.device).reshape(3, 3)
        h, S = y @ C.T, C @ S
    H = torch.zeros(B, 3, nstate, dtype=p.dtype, device=p.device)
    H[:, :, 6:9] = S
    return _vec(z, p) - h, H


def range_to(nominal, rot, z, beacon, lever=None, nstate=18):
    """An acoustic range from the transponder to a beacon at a known world position, one row.  beacon: (3,) or (B, 3); lever: the
    transponder's position in the IMU frame; None = 0.
        d = p + R lever - beacon        h(x) = |d|        H = (d / |d|)' [ I | -R [lever]x ] on the p and theta columns, every other 0
    z: (B,) or (B, 1).  Returns res (B, 1), H (B, 1, nstate).  (|d| = 0 has no direction: the row is then not finite and
    correct_rows leaves that filter untouched.)"""
    p, R = _parts(nominal, rot, nstate)
    B = p.shape[0]
    d = p - _vec(beacon, p)
    lv = None
    if lever is not None:
        lv = _vec(lever, p).expand(B, 3)
        d = d + torch.einsum("bij,bj->bi", R, lv)
    rng = torch.linalg.vector_norm(d, dim=1, keepdim=True)
    e = d / rng
    H = torch.zeros(B, 1, nstate, dtype=p.dtype, device=p.device)
    H[:, 0, 0:3] = e
    if lv is not None:
        H[:, 0, 6:9] = -torch.einsum("bi,bij->bj", e, R @ _skew(lv))
    return torch.as_tensor(z, dtype=p.dtype, device=p.device).reshape(B, 1) - rng, H
