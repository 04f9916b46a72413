"""Rigid poses [R t; 0 1], x' = R x + t, applied to clouds: plain torch, on CPU tensors too.  register produces such
poses, frame produces and applies them; both import this module at the top."""
import torch

from ._cloud import normal_column


def check_pose(pose, what):
    """-> fp64 [4, 4] on the CPU, finite, last row (0, 0, 0, 1)"""
    try:
        p = torch.as_tensor(pose).detach().to("cpu", torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{what}: a 4 x 4 matrix, got {pose!r}")
    if p.shape != (4, 4):
        raise ValueError(f"{what}: a 4 x 4 matrix, got shape {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError(f"{what}: entries must be finite")
    if p[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError(f"{what}: the last row must be (0, 0, 0, 1), got {p[3].tolist()}")
    return p


def apply_pose(pcl, pose, normal_col="auto"):
    """pcl [N, C >= 3], columns 0:3 the position; pose 4 x 4, x' = R x + t -> a copy of the cloud with the position moved
    and the normal columns rotated (normal_col as voxel_downsample takes it: 'auto' is 6 when C == 9, else none).  fp64
    arithmetic, one rounding to the cloud's type.  Plain torch: it also runs on CPU tensors."""
    if not isinstance(pcl, torch.Tensor) or pcl.dim() != 2 or pcl.shape[1] < 3:
        raise ValueError("apply_pose: a tensor [N, >= 3]")
    if not pcl.dtype.is_floating_point:
        raise ValueError(f"apply_pose: a floating-point cloud, got {pcl.dtype}")
    if isinstance(pose, torch.Tensor) and pose.is_cuda and pose.shape == (4, 4):
        T = pose.detach().to(pcl.device, torch.float64)          # a registration's pose: no read-back
    else:
        T = check_pose(pose, "apply_pose: pose").to(pcl.device)
    nc = normal_column(normal_col, pcl.shape[1])
    R, t = T[:3, :3], T[:3, 3]
    out = pcl.detach().clone()
    out[:, :3] = (pcl[:, :3].to(torch.float64) @ R.T + t).to(pcl.dtype)
    if nc >= 0:
        out[:, nc:nc + 3] = (pcl[:, nc:nc + 3].to(torch.float64) @ R.T).to(pcl.dtype)
    return out


def inverse_pose(pose):
    """the inverse of a rigid pose [R t; 0 1]: [R^T, -R^T t; 0 1], fp64, on the pose's device"""
    T = pose.detach().to(torch.float64) if isinstance(pose, torch.Tensor) else check_pose(pose, "inverse_pose")
    out = torch.eye(4, dtype=torch.float64, device=T.device)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out
