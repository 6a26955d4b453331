"""The per-sample training transforms of pointcept/datasets/transform.py on the device, under the reference's names and
constructor signatures (``TRANSFORMS.build(dict(type="RandomRotate", axis="z", ...))``), for dicts of GPU tensors.

Two things differ from the reference by design:

* **Draw and apply are separate.**  ``draw(rng, data_dict) -> params`` takes every random decision of one call from a
  ``numpy.random.Generator`` (owned by ``Compose``; no global ``random`` / ``np.random`` state, no device sync) and returns a
  small plain dict: fired flag, angle, scale, flips, blend, translation, a 64-bit seed for per-point noise.  ``apply(data_dict,
  params)`` does the work, ``__call__`` is ``apply(draw(...))``.  Replaying recorded parameters (``noise=`` / ``idx=`` entries
  replace a seed) makes every op comparable with the reference although the device draws its own numbers.
* **Compose fuses.**  A run of CenterShift / RandomRotate / RandomRotateTargetAngle / RandomScale / RandomShift / RandomFlip /
  RandomJitter is folded on the host into one fp64 affine ``A x + b``, one rotation quaternion, a reflection and a scale factor and
  applied in ONE ``ss_aug_gaussians`` pass over coord / quat / scale / normal.  Ops that need the bounding box of the *current*
  coordinates (CenterShift, rotations with ``center=None``) call ``ss_aug_bbox`` with the pending affine: that is a 6-float
  device -> host readback (a sync) per such op, and no pass over memory is spent on flushing.  The pass is flushed at the first
  op outside the family, when a rotation follows a flip or a jitter (the kernel rotates first), or when a second flip or jitter
  arrives.  A run of ChromaticAutoContrast / ChromaticTranslation / ChromaticJitter / NormalizeColor in that order is one
  ``ss_aug_color`` pass.  RandomColorJitter / RandomColorGrayScale (the self-supervised view lists) are a family of their own:
  their fired steps queue up, in any order, for ONE ``ss_color_chain`` pass.  ``Compose(fuse=False)`` runs op by op.

``pc_coord`` / ``pc_segment`` (the point cloud some val / test lists carry beside the Gaussians) follow the reference: CenterShift, the
rotations, RandomScale and RandomFlip move the cloud with the Gaussians (a second pending affine, one more ``ss_aug_gaussians`` launch
per flush), ``GridSample(apply_to_pc=True)`` keeps one point per occupied cell of the cloud's own grid, every other op passes both keys through.

The alternatives the shipped lists carry commented out, and the rest of the reference's per-sample transforms, are here too:
NormalizeCoord and PositiveShift fold into the pending affine (``RigidState.moments`` is to NormalizeCoord what ``bbox`` is to
CenterShift: an fp64 reduction of the pending ``A x + b``, a 4-double readback), HueSaturationTranslation is one ``ss_aug_hsv`` pass
(the reference's fp64 HSV round trip, bit for bit), InstanceParser two kernels over a sorted CSR of the instance ids; RandomColorDrop,
PointClip, ShufflePoint, CropBoundary, Add and ContrastiveViewsGenerator need no kernel of their own.

All ops work IN PLACE on float32 contiguous tensors (as the reference mutates its arrays) and refuse CPU tensors: there is no
CPU fallback.  ``draw``, the host composition (``RigidState`` with a ``bbox_fn``) and ``box_blur3`` need no device.
"""
import copy
import numbers

import numpy as np
import torch

from .. import gpu_transforms as gt
from .. import native as nv
from .registry import TRANSFORMS


# ---- host quaternion helpers (fp64, wxyz) ---------------------------------------------------------------------------------------
def quat_mul(p, q):
    """Hamilton product p (x) q, wxyz."""
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.array([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw], dtype=np.float64)


def quat_from_matrix(m):
    """Rotation matrix -> unit quaternion (wxyz) with the sign scipy's Rotation.from_matrix gives: the branch is the arg-max of
    [M00, M11, M22, trace] and the component it selects (x / y / z / w) comes out positive."""
    m = np.asarray(m, dtype=np.float64)
    dec = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
    c = int(np.argmax(dec))
    q = np.empty(4)                                           # xyzw while it is built
    if c != 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - dec[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    else:
        q[0] = m[2, 1] - m[1, 2]
        q[1] = m[0, 2] - m[2, 0]
        q[2] = m[1, 0] - m[0, 1]
        q[3] = 1 + dec[3]
    q /= np.linalg.norm(q)
    return np.array([q[3], q[0], q[1], q[2]])


def axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)
    if axis == "z":
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    raise NotImplementedError("axis must be 'x', 'y' or 'z'")


def box_blur3(noise, rounds=2):
    """ElasticDistortion's smoothing (transform.py:1135-1154): the 3-tap box blur (1/3, 1/3, 1/3) along x, then y, then z with
    zero padding, `rounds` times, on a (d0, d1, d2, C) float32 tensor of any device."""
    third = noise.new_tensor(1.0 / 3.0)
    for _ in range(rounds):
        for dim in (0, 1, 2):
            pad = torch.zeros_like(noise.narrow(dim, 0, 1))
            ext = torch.cat([pad, noise, pad], dim=dim)
            d = noise.shape[dim]
            noise = (ext.narrow(dim, 0, d) + ext.narrow(dim, 1, d) + ext.narrow(dim, 2, d)) * third
    return noise


def _seed(rng):
    return int(rng.integers(0, 1 << 63))


def _dev(t, name, cols=None):
    """The tensors the kernels update in place: float32, contiguous, on the GPU."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: scenesplat_amd transforms need a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name}: must be a contiguous float32 tensor (it is updated in place)")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise RuntimeError(f"{name}: expected (n, {cols}), got {tuple(t.shape)}")
    return t


def _has_pc(data_dict):
    """the reference treats pc_coord inside its `if "coord" in data_dict` branches: both keys, or the cloud is left alone"""
    return "coord" in data_dict and "pc_coord" in data_dict


def _noise_arg(noise, like):
    """A recorded (n, 3) N(0,1) array / tensor -> float32 device tensor."""
    if noise is None:
        return None
    return torch.as_tensor(np.asarray(noise, dtype=np.float32) if not isinstance(noise, torch.Tensor) else noise,
                           dtype=torch.float32).to(like.device).contiguous()


# ---- the pending rigid transform ------------------------------------------------------------------------------------------------
class RigidState:
    """What a run of rigid ops has folded so far: coord -> A x + b (fp64), quaternion -> q (x) quat then the flip conjugation,
    scale -> scale * smul, normal -> L normal, then the jitter.  bbox_fn(A, b) -> 6 floats overrides the device bounding box
    (host-only composition: tests, dry runs).
    pc_coord (the point cloud some lists carry beside the Gaussians) -> A_pc x + b_pc: the ops that treat it in the reference
    (CenterShift, the rotations, RandomScale, RandomFlip) fold into it with `pc=True`, with the Gaussians' shift and centre;
    RandomShift and RandomJitter do not, so the two affines differ after them.  The flush rules are shared."""
    family = "rigid"

    def __init__(self, bbox_fn=None, moments_fn=None):
        self.bbox_fn = bbox_fn
        self.moments_fn = moments_fn      # (A, b) -> {mean xyz, largest squared norm}: the host stand-in of moments(), as bbox_fn is of bbox()
        self.reset()

    def reset(self):
        self.A, self.b, self.L = np.eye(3), np.zeros(3), np.eye(3)
        self.A_pc, self.b_pc = np.eye(3), np.zeros(3)
        self.q = None                 # composed rotation quaternion (wxyz), None = no rotation yet
        self.flip = 0                 # bit 0: x, bit 1: y
        self.smul = np.ones(3)
        self.scaled = False
        self.jitter = None            # dict(sigma, clip, seed | noise)

    def coord_pending(self):
        return not (np.array_equal(self.A, np.eye(3)) and not self.b.any())

    def affine12(self):
        return None if not self.coord_pending() else list(self.A.reshape(-1)) + list(self.b)

    def pc_pending(self):
        return not (np.array_equal(self.A_pc, np.eye(3)) and not self.b_pc.any())

    def affine12_pc(self):
        return None if not self.pc_pending() else list(self.A_pc.reshape(-1)) + list(self.b_pc)

    def bbox(self, data):
        """Bounding box {min xyz, max xyz} of the current coordinates, pending affine included (6-float readback)."""
        if self.jitter is not None:
            self.flush(data)
        if self.bbox_fn is not None:
            return np.asarray(self.bbox_fn(self.A, self.b), dtype=np.float64)
        return nv.aug_bbox(_dev(data["coord"], "coord", 3), self.affine12()).cpu().numpy().astype(np.float64)

    def moments(self, data):
        """{mean xyz, largest squared norm} of the current coordinates in fp64, pending affine included (ss_aug_moments: a 4-double
        readback)."""
        if self.jitter is not None:
            self.flush(data)
        if self.moments_fn is not None:
            return np.asarray(self.moments_fn(self.A, self.b), dtype=np.float64)
        coord = _dev(data["coord"], "coord", 3)
        m = nv.aug_moments(coord, self.affine12()).cpu().numpy()
        m[:3] /= coord.shape[0]
        return m

    def before_coord_op(self, data):
        if self.jitter is not None:           # the kernel adds the jitter last
            self.flush(data)

    def shift(self, data, t, pc=False):
        self.before_coord_op(data)
        self.b = self.b + np.asarray(t, dtype=np.float64)
        if pc:
            self.b_pc = self.b_pc + np.asarray(t, dtype=np.float64)

    def rotate(self, data, rot, center, has_coord, pc=False):
        if self.flip or self.jitter is not None:          # the kernel rotates before it flips
            self.flush(data)
        if has_coord:
            if center is None:
                bb = self.bbox(data)
                center = (bb[:3] + bb[3:]) / 2
            center = np.asarray(center, dtype=np.float64)
            self.A = rot @ self.A
            self.b = rot @ (self.b - center) + center
            if pc:                                        # about the SAME centre: the Gaussians' (transform.py:577-580)
                self.A_pc = rot @ self.A_pc
                self.b_pc = rot @ (self.b_pc - center) + center
        self.L = rot @ self.L
        r = quat_from_matrix(rot)
        self.q = r if self.q is None else quat_mul(r, self.q)

    def scale(self, data, s, pc=False):
        self.before_coord_op(data)
        s = np.broadcast_to(np.asarray(s, dtype=np.float64), (3,))
        self.A = s[:, None] * self.A
        self.b = s * self.b
        if pc:
            self.A_pc = s[:, None] * self.A_pc
            self.b_pc = s * self.b_pc
        self.smul = self.smul * s
        self.scaled = True

    def reflect(self, data, flip_x, flip_y, pc=False):
        if not (flip_x or flip_y):
            return
        if self.flip or self.jitter is not None:          # one conjugation + sign rule per pass
            self.flush(data)
        f = np.array([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
        self.A = f[:, None] * self.A
        self.b = f * self.b
        self.L = f[:, None] * self.L
        if pc:
            self.A_pc = f[:, None] * self.A_pc
            self.b_pc = f * self.b_pc
        self.flip = (1 if flip_x else 0) | (2 if flip_y else 0)

    def add_jitter(self, data, sigma, clip, seed=0, noise=None):
        if self.jitter is not None:
            self.flush(data)
        self.jitter = dict(sigma=sigma, clip=clip, seed=seed, noise=noise)

    def flush(self, data):
        """ONE ss_aug_gaussians pass over the arrays the pending ops touch, and one more over pc_coord when they touched the cloud."""
        aff, aff_pc = self.affine12(), self.affine12_pc()
        pc = _dev(data["pc_coord"], "pc_coord", 3) if aff_pc is not None and "pc_coord" in data else None
        coord = data.get("coord") if (aff is not None or self.jitter is not None) else None
        quat = data.get("quat") if (self.q is not None or self.flip) else None
        scale = data.get("scale") if self.scaled else None
        normal = data.get("normal") if not np.array_equal(self.L, np.eye(3)) else None
        j = self.jitter
        if coord is not None or quat is not None or scale is not None or normal is not None:
            nv.aug_gaussians_(
                coord=None if coord is None else _dev(coord, "coord", 3), quat=None if quat is None else _dev(quat, "quat", 4),
                scale=None if scale is None else _dev(scale, "scale", 3), normal=None if normal is None else _dev(normal, "normal", 3),
                affine=aff, rquat=None if self.q is None else list(self.q), flip=self.flip, scale_mul=list(self.smul),
                lin=list(self.L.reshape(-1)), jitter=None if j is None or coord is None else (j["sigma"], j["clip"]),
                noise=None if j is None or coord is None else _noise_arg(j["noise"], coord), seed=0 if j is None else j["seed"])
        if pc is not None:
            nv.aug_gaussians_(coord=pc, affine=aff_pc)
        self.reset()


class ColorState:
    """Pending colour steps in the kernel's order: contrast (1) -> translation (2) -> jitter (3) -> normalize (4)."""
    family = "color"

    def __init__(self):
        self.reset()

    def reset(self):
        self.stage, self.flags, self.normalize = 0, 0, False
        self.lo = self.hi = self.tr = self.noise = None
        self.blend, self.std, self.seed = 0.0, 0.0, 0

    def enter(self, data, stage):
        if self.stage >= stage:
            self.flush(data)
        self.stage = stage

    def flush(self, data):
        if (self.flags or self.normalize) and "color" in data:
            c = _dev(data["color"], "color", 3)
            nv.aug_color_(c, self.flags, self.lo, self.hi, self.blend, self.tr, self.std, _noise_arg(self.noise, c), self.seed,
                          self.normalize)
        self.reset()


class ChainState:
    """Pending (code, factor) steps of RandomColorJitter / RandomColorGrayScale, in the order they were drawn: one ss_color_chain
    pass at the flush (plus one reduction pass per contrast step).  The kernel takes 8 steps; a ninth flushes first."""
    family = "chain"

    def __init__(self):
        self.steps = []

    def add(self, data, code, factor=0.0):
        if len(self.steps) == nv.CHAIN_MAX_STEPS:
            self.flush(data)
        self.steps.append((code, float(factor)))

    def flush(self, data):
        if self.steps and "color" in data:
            nv.color_chain_(_dev(data["color"], "color", 3), self.steps)
        self.steps = []


_STATES = dict(rigid=RigidState, color=ColorState, chain=ChainState)


class Transform:
    """Base: draw() takes the random decisions, apply() does the work; ops with a `family` can also fold() into a pending pass."""
    family = None

    def draw(self, rng, data_dict):
        return {}

    def fold(self, state, data_dict, params):
        raise NotImplementedError

    def apply(self, data_dict, params):
        state = _STATES[self.family]()
        self.fold(state, data_dict, params)
        state.flush(data_dict)
        return data_dict

    def __call__(self, data_dict, rng=None):
        return self.apply(data_dict, self.draw(np.random.default_rng() if rng is None else rng, data_dict))


# ---- rigid family ---------------------------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class CenterShift(Transform):
    """transform.py:446-465: x, y to the centre of the bounding box, z to its floor (apply_z) or untouched; pc_coord gets the
    same shift (the Gaussians' box, not its own)."""
    family = "rigid"

    def __init__(self, apply_z=True):
        self.apply_z = apply_z

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            bb = state.bbox(data_dict)
            state.shift(data_dict, [-(bb[0] + bb[3]) / 2, -(bb[1] + bb[4]) / 2, -bb[2] if self.apply_z else 0.0],
                        pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomShift(Transform):
    family = "rigid"

    def __init__(self, shift=((-0.2, 0.2), (-0.2, 0.2), (0, 0))):
        self.shift = shift

    def draw(self, rng, data_dict):
        return dict(shift=[float(rng.uniform(lo, hi)) for lo, hi in self.shift])

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.shift(data_dict, params["shift"])


@TRANSFORMS.register_module()
class RandomRotate(Transform):
    """transform.py:544-601: rotates coord about `center` (None: the bounding-box centre of the current coordinates), the
    Gaussians' quaternions (left-multiplied) and the normals; pc_coord about the same centre."""
    family = "rigid"

    def __init__(self, angle=None, center=None, axis="z", always_apply=False, p=0.5):
        self.angle = [-1, 1] if angle is None else angle
        self.axis = axis
        self.always_apply = always_apply
        self.p = p if not self.always_apply else 1
        self.center = center
        axis_rotation(axis, 0.0)

    def draw(self, rng, data_dict):
        if rng.random() > self.p:
            return dict(fired=False)
        return dict(fired=True, angle=float(rng.uniform(self.angle[0], self.angle[1]) * np.pi))

    def fold(self, state, data_dict, params):
        if params["fired"]:
            state.rotate(data_dict, axis_rotation(self.axis, params["angle"]), self.center, "coord" in data_dict,
                         pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomRotateTargetAngle(RandomRotate):
    """transform.py:604-659: as RandomRotate with the angle taken from a list (multiples of pi)."""

    def __init__(self, angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75):
        super().__init__(angle=angle, center=center, axis=axis, always_apply=always_apply, p=p)

    def draw(self, rng, data_dict):
        if rng.random() > self.p:
            return dict(fired=False)
        return dict(fired=True, angle=float(rng.choice(np.asarray(self.angle, dtype=np.float64)) * np.pi))


@TRANSFORMS.register_module()
class RandomScale(Transform):
    """transform.py:662-678: coord, pc_coord and the Gaussians' `scale` are multiplied by the same draw."""
    family = "rigid"

    def __init__(self, scale=None, anisotropic=False):
        self.scale = scale if scale is not None else [0.95, 1.05]
        self.anisotropic = anisotropic

    def draw(self, rng, data_dict):
        return dict(scale=rng.uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1).tolist())

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.scale(data_dict, params["scale"], pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomFlip(Transform):
    """transform.py:681-727: mirrors x and / or y of coord, pc_coord and normal; the quaternions get the conjugation F R F."""
    family = "rigid"

    def __init__(self, p=0.5):
        self.p = p

    def draw(self, rng, data_dict):
        return dict(flip_x=bool(rng.random() < self.p), flip_y=bool(rng.random() < self.p))

    def fold(self, state, data_dict, params):
        state.reflect(data_dict, params["flip_x"], params["flip_y"], pc=_has_pc(data_dict))


@TRANSFORMS.register_module()
class RandomJitter(Transform):
    """transform.py:730-745: coord += clip(sigma N(0,1), +-clip); params["noise"] (n, 3) replays recorded draws."""
    family = "rigid"

    def __init__(self, sigma=0.01, clip=0.05):
        assert clip > 0
        self.sigma = sigma
        self.clip = clip

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.add_jitter(data_dict, self.sigma, self.clip, params.get("seed", 0), params.get("noise"))


# ---- colour family --------------------------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class ChromaticAutoContrast(Transform):
    """transform.py:769-787; the per-channel lo / hi come from ss_aug_bbox on the colours (6-float readback)."""
    family = "color"

    def __init__(self, p=0.2, blend_factor=None):
        self.p = p
        self.blend_factor = blend_factor

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, blend=float(rng.random() if self.blend_factor is None else self.blend_factor))

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 1)
            bb = nv.aug_bbox(_dev(data_dict["color"], "color", 3)).cpu().numpy()
            if not (bb[3:] > bb[:3]).all():                   # the reference divides by hi - lo = 0 here and fills the channel with NaN
                raise ValueError("ChromaticAutoContrast: a colour channel is constant over the sample")
            state.lo, state.hi, state.blend = bb[:3].tolist(), bb[3:].tolist(), params["blend"]
            state.flags |= nv.AUG_COLOR_CONTRAST


@TRANSFORMS.register_module()
class ChromaticTranslation(Transform):
    """transform.py:790-800"""
    family = "color"

    def __init__(self, p=0.95, ratio=0.05):
        self.p = p
        self.ratio = ratio

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, tr=((rng.random(3) - 0.5) * 255 * 2 * self.ratio).tolist())

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 2)
            state.tr = list(params["tr"])
            state.flags |= nv.AUG_COLOR_TRANSLATE


@TRANSFORMS.register_module()
class ChromaticJitter(Transform):
    """transform.py:803-816; params["noise"] (n, 3) replays recorded draws."""
    family = "color"

    def __init__(self, p=0.95, std=0.005):
        self.p = p
        self.std = std

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False)
        return dict(fired=True, seed=_seed(rng))

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.enter(data_dict, 3)
            state.std, state.seed, state.noise = self.std, params.get("seed", 0), params.get("noise")
            state.flags |= nv.AUG_COLOR_JITTER


@TRANSFORMS.register_module()
class NormalizeColor(Transform):
    """transform.py:415-420: color / 127.5 - 1"""
    family = "color"

    def fold(self, state, data_dict, params):
        if "color" in data_dict:
            state.enter(data_dict, 4)
            state.normalize = True


# ---- ops with a pass of their own -----------------------------------------------------------------------------------------------
@TRANSFORMS.register_module()
class ElasticDistortion(Transform):
    """transform.py:1120-1178.  Per (granularity, magnitude) pair: bounding box of the current coordinates (6-float readback),
    a (dims, 3) N(0,1) grid smoothed by box_blur3, one ss_aug_elastic pass.  The grid's shape depends on the box the pass sees --
    the second pair sees the first one's output -- so draw() hands over the seed the grids are drawn from (host Generator, at
    apply time); params["noise"] = [raw grid per pair] replays recorded grids instead."""

    def __init__(self, distortion_params=None):
        self.distortion_params = [[0.2, 0.4], [0.8, 1.6]] if distortion_params is None else distortion_params

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < 0.95), seed=_seed(rng))

    @staticmethod
    def grid_geometry(bbox, granularity):
        """(noise_dim (3,) int, origin (3,) f32) from the fp32 box of the coordinates (transform.py:1138-1164)."""
        bb = np.asarray(bbox, dtype=np.float32)
        lo, hi = bb[:3], bb[3:]
        dim = np.floor_divide(hi - lo, np.float32(granularity)).astype(int) + 3
        return dim, lo - np.float32(granularity)

    def apply(self, data_dict, params):
        if "coord" not in data_dict or self.distortion_params is None or not params["fired"]:
            return data_dict
        coord = _dev(data_dict["coord"], "coord", 3)
        grids = params.get("noise")
        rng = None if grids is not None else np.random.default_rng(params["seed"])
        for k, (granularity, magnitude) in enumerate(self.distortion_params):
            dim, origin = self.grid_geometry(nv.aug_bbox(coord).cpu().numpy(), granularity)
            if grids is not None:
                raw = torch.as_tensor(np.asarray(grids[k], dtype=np.float32))
                if tuple(raw.shape) != (*dim.tolist(), 3):
                    raise ValueError(f"ElasticDistortion: recorded grid {tuple(raw.shape)} does not fit the box ({dim.tolist()})")
            else:
                raw = torch.from_numpy(rng.standard_normal((*dim.tolist(), 3), dtype=np.float32))
            noise = box_blur3(raw.to(coord.device)).contiguous()
            nv.aug_elastic_(coord, noise, origin.tolist(), granularity, magnitude)
        return data_dict


# the per-point entries RandomDropout subsets (transform.py:518-540)
DROPOUT_KEYS = ("coord", "color", "normal", "strength", "segment", "instance", "quat", "scale", "opacity", "lang_feat",
                "valid_feat_mask")


@TRANSFORMS.register_module()
class RandomDropout(Transform):
    """transform.py:497-541: keep int(n (1 - ratio)) random rows (randperm, unsorted as np.random.choice), of exactly the keys
    the reference subsets; `sampled_index` rows are always kept and remapped.  params["idx"] replays a recorded index."""

    def __init__(self, dropout_ratio=0.2, dropout_application_ratio=0.5):
        self.dropout_ratio = dropout_ratio
        self.dropout_application_ratio = dropout_application_ratio

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < self.dropout_application_ratio), seed=_seed(rng))

    def apply(self, data_dict, params):
        if not params["fired"]:
            return data_dict
        coord = data_dict["coord"]
        if not isinstance(coord, torch.Tensor) or not coord.is_cuda:
            raise RuntimeError("RandomDropout: GPU tensors required (no CPU fallback)")
        n = coord.shape[0]
        if params.get("idx") is not None:
            idx = torch.as_tensor(np.asarray(params["idx"]), dtype=torch.int64).to(coord.device)
        else:
            g = torch.Generator(device=coord.device)
            g.manual_seed(int(params["seed"]))
            idx = torch.randperm(n, device=coord.device, generator=g)[:int(n * (1 - self.dropout_ratio))]
        if "sampled_index" in data_dict:
            si = data_dict["sampled_index"].long()
            idx = torch.unique(torch.cat([idx, si]))
            mask = torch.zeros(n, dtype=torch.bool, device=coord.device)
            mask[si] = True
            data_dict["sampled_index"] = torch.nonzero(mask[idx]).reshape(-1)
        idx32 = idx.to(torch.int32).contiguous()
        for k in DROPOUT_KEYS:
            v = data_dict.get(k)
            if isinstance(v, torch.Tensor):
                data_dict[k] = gt.take_rows(v, idx32)
        return data_dict


@TRANSFORMS.register_module()
class ToTensor(Transform):
    """transform.py:374-399 for data that already lives in tensors: a pass-through (host arrays are the dataset's business)."""

    def apply(self, data_dict, params):
        return data_dict


@TRANSFORMS.register_module()
class Copy(Transform):
    """transform.py:355-371"""

    def __init__(self, keys_dict=None):
        self.keys_dict = dict(coord="origin_coord", segment="origin_segment") if keys_dict is None else keys_dict

    def apply(self, data_dict, params):
        for key, value in self.keys_dict.items():
            if key in data_dict:
                v = data_dict[key]
                data_dict[value] = v.clone().detach() if isinstance(v, torch.Tensor) else copy.deepcopy(v)
        return data_dict


@TRANSFORMS.register_module()
class GridSample(Transform):
    """GridSample(mode="train") (transform.py:1181-1300) over gpu_transforms.grid_sample_train: one random point per occupied voxel,
    `keys` subset to it.  draw() hands the device generator its seed; params["idx"] replays a recorded per-voxel pick.
    `sampled_index` rows are always kept and remapped (as in RandomDropout).  With apply_to_pc, pc_coord / pc_segment are
    subset to one point per occupied cell of the cloud's own grid (gpu_transforms.grid_sample_pc), in ascending cell order --
    the reference emits the same rows in the order of its FNV hashes."""

    def __init__(self, grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"),
                 return_inverse=False, return_grid_coord=False, return_min_coord=False, return_displacement=False,
                 project_displacement=False, importance_sample_key=None, apply_to_pc=True):
        if mode != "train":
            raise NotImplementedError('GridSample: only mode="train" is registered (gpu_transforms.grid_sample_test serves the tester)')
        if return_min_coord or return_displacement or project_displacement or importance_sample_key is not None:
            raise NotImplementedError("GridSample: min_coord / displacement / importance sampling have no device form")
        self.grid_size, self.hash_type, self.mode, self.keys = grid_size, hash_type, mode, keys     # voxel keys are exact: no hash
        self.return_inverse, self.return_grid_coord, self.apply_to_pc = return_inverse, return_grid_coord, apply_to_pc

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def apply(self, data_dict, params):
        coord = data_dict["coord"]
        if not isinstance(coord, torch.Tensor) or not coord.is_cuda:
            raise RuntimeError("GridSample: GPU tensors required (no CPU fallback)")
        if "pc_coord" in data_dict and self.apply_to_pc:
            pc = _dev(data_dict["pc_coord"], "pc_coord", 3)
            seg = data_dict.get("pc_segment")
            if seg is not None and seg.shape[0] != pc.shape[0]:
                raise ValueError(f"GridSample: pc_segment has {seg.shape[0]} rows, pc_coord has {pc.shape[0]}")
            chosen = gt.grid_sample_pc(pc, self.grid_size, seg)
            data_dict["pc_coord"] = pc[chosen]
            if seg is not None:
                data_dict["pc_segment"] = seg[chosen]
        g = torch.Generator(device=coord.device)
        g.manual_seed(int(params.get("seed", 0)))
        idx = params.get("idx")
        if idx is not None:
            idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).to(coord.device)
        out = gt.grid_sample_train(coord, self.grid_size, generator=g, return_inverse=self.return_inverse,
                                   sampled_index=data_dict.get("sampled_index"), idx_unique=idx)
        idx32 = out["idx_unique"].to(torch.int32).contiguous()
        if "sampled_index" in out:
            data_dict["sampled_index"] = out["sampled_index"]
        if self.return_inverse:
            data_dict["inverse"] = out["inverse"]
        if self.return_grid_coord:
            data_dict["grid_coord"] = out["grid_coord"]
        for k in self.keys:
            if k in data_dict:
                data_dict[k] = gt.take_rows(data_dict[k], idx32)
        return data_dict


@TRANSFORMS.register_module()
class SphereCrop(Transform):
    """transform.py:1419-1548 over gpu_transforms.sphere_crop; params["center_index"] replays a recorded centre."""

    def __init__(self, point_max=80000, sample_rate=None, mode="random"):
        assert mode in ["random", "center", "all"]
        self.point_max, self.sample_rate, self.mode = point_max, sample_rate, mode

    def draw(self, rng, data_dict):
        return dict(u=float(rng.random()))

    def apply(self, data_dict, params):
        ci = params.get("center_index")
        if ci is None and self.mode == "random":
            ci = min(int(params["u"] * data_dict["coord"].shape[0]), data_dict["coord"].shape[0] - 1)
        return gt.sphere_crop(data_dict, self.point_max, self.sample_rate, self.mode, center_index=ci)


@TRANSFORMS.register_module()
class Collect(Transform):
    """transform.py:319-352 over gpu_transforms.collect"""

    def __init__(self, keys, offset_keys_dict=None, **kwargs):
        self.keys, self.offset_keys, self.kwargs = keys, offset_keys_dict, kwargs

    def apply(self, data_dict, params):
        return gt.collect(data_dict, self.keys, self.offset_keys, **self.kwargs)


# ---- the self-supervised view generator (transform.py:18-315, 820-1032) ---------------------------------------------------------
@TRANSFORMS.register_module()
class RandomColorGrayScale(Transform):
    """transform.py:819-848: with probability p all three channels become 0.2989 r + 0.587 g + 0.114 b."""
    family = "chain"

    def __init__(self, p):
        self.p = p

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < self.p))

    def fold(self, state, data_dict, params):
        if params["fired"] and "color" in data_dict:
            state.add(data_dict, nv.CHAIN_GRAY)


@TRANSFORMS.register_module()
class RandomColorJitter(Transform):
    """transform.py:851-1032 (after torchvision): brightness / contrast / saturation / hue in a drawn order, each applied with
    probability p.  draw() -> order (a permutation of 0..3 = brightness, contrast, saturation, hue) and the four factors; a factor
    is None when its range is None or its own `rand() < p` did not fire -- only steps that have a range consume a p draw, as in
    the reference's __call__.  The fired steps are ONE ss_color_chain pass (and fold into the pass of a neighbouring
    RandomColorGrayScale under Compose(fuse=True))."""
    family = "chain"
    NAMES = ("brightness", "contrast", "saturation", "hue")
    CODES = (nv.CHAIN_BRIGHTNESS, nv.CHAIN_CONTRAST, nv.CHAIN_SATURATION, nv.CHAIN_HUE)

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, p=0.95):
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        self.hue = self._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.p = p

    @staticmethod
    def _check_input(value, name, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError("If {} is a single number, it must be non negative.".format(name))
            value = [center - float(value), center + float(value)]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not bound[0] <= value[0] <= value[1] <= bound[1]:
                raise ValueError("{} values should be between {}".format(name, bound))
        else:
            raise TypeError("{} should be a single number or a list/tuple with length 2.".format(name))
        if value[0] == value[1] == center:      # 0 or (1, 1) for brightness / contrast / saturation, (0, 0) for hue: nothing to do
            value = None
        return value

    def draw(self, rng, data_dict):
        order = [int(i) for i in rng.permutation(4)]
        ranges = (self.brightness, self.contrast, self.saturation, self.hue)
        factors = [None if r is None else float(rng.uniform(r[0], r[1])) for r in ranges]
        for i in order:                                    # the per-step coin, in the order the steps run
            if factors[i] is not None and not rng.random() < self.p:
                factors[i] = None
        return dict(order=order, **dict(zip(self.NAMES, factors)))

    def fold(self, state, data_dict, params):
        if "color" not in data_dict:
            return
        for i in params["order"]:
            f = params[self.NAMES[int(i)]]
            if f is None:
                continue
            if int(i) == 3 and not -0.5 <= f <= 0.5:
                raise ValueError("hue_factor ({}) is not in [-0.5, 0.5].".format(f))
            if int(i) != 3 and f < 0:
                raise ValueError("{}_factor ({}) is not non-negative.".format(self.NAMES[int(i)], f))
            state.add(data_dict, self.CODES[int(i)], f)


@TRANSFORMS.register_module()
class RandomColorSolarize(Transform):
    """transform.py:178-194.  Registered, and it draws as the reference does (one rand() when `color` is there), but it leaves
    `color` UNCHANGED: the reference computes the solarized colours into a local and returns data_dict without storing them,
    so the shipped lists train on unsolarized views.  This class reproduces that; there is nothing to launch."""

    def __init__(self, p=0.2, threshold=128):
        self.p, self.threshold = p, threshold

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < self.p)) if "color" in data_dict else dict(fired=False)

    def apply(self, data_dict, params):
        return data_dict


# the per-point entries SphereCropRandomMaxPoints crops (transform.py:221-254): SphereCrop's and two more
_CROP_MAX_POINTS_EXTRA = ("sh", "lang_feat_64")


@TRANSFORMS.register_module()
class SphereCropRandomMaxPoints(Transform):
    """transform.py:197-255: point_max' = int(uniform(random_scale) * point_max); a sample with more points keeps the point_max'
    nearest to a random point of it, in ascending-distance order (gpu_transforms.sphere_crop: ties by row index).
    params["point_max"] / params["center_index"] replay a recorded call."""

    def __init__(self, random_scale=(0.5, 1.0), point_max=80000):
        self.random_scale, self.point_max = random_scale, point_max

    def draw(self, rng, data_dict):
        return dict(point_max=int(rng.uniform(self.random_scale[0], self.random_scale[1]) * self.point_max), u=float(rng.random()))

    def apply(self, data_dict, params):
        assert "coord" in data_dict
        n = data_dict["coord"].shape[0]
        ci = params.get("center_index")
        if ci is None:
            ci = min(int(params["u"] * n), n - 1)
        return gt.sphere_crop(data_dict, int(params["point_max"]), None, "random", center_index=ci, extra_keys=_CROP_MAX_POINTS_EXTRA)


@TRANSFORMS.register_module()
class GSGaussianBlurVoxelOpc(Transform):
    """transform.py:60-176: with probability p, the rows with opacity > 0.5 get `color` and the `extra_keys` among opacity / scale /
    quat / normal replaced by the Gaussian-weighted mean (sigma ~ U(sigma[0], sigma[1]), truncate 2.0, scipy's `reflect` border)
    over the masked voxels around them; with "quat" in extra_keys every row of quat is then normalised.  The reference fills a
    DENSE grid over the view's bounding box for this; ss_voxel_blur hashes the occupied voxels and gathers (O(n) memory, no
    readback).  Needs `grid_coord` (a GridSample with return_grid_coord in front) with UNIQUE rows -- one point per voxel, which
    GridSample guarantees; with duplicates the reference keeps the last row written into a cell, the hash the first inserted.
    Limits of the kernel: r = int(2 sigma + 0.5) <= 8, so the constructor refuses a sigma range that reaches 4.25; and a view
    whose grid_coord spans 2^21 cells or more on an axis is left UNBLURRED (the normalisation of quat still runs) -- the kernel
    says so in a device status word that apply() does not read, since reading it is a host sync.  GridSample refuses such an
    extent itself, so a grid_coord that comes from it never gets there."""
    KEYS = ("opacity", "scale", "quat", "normal")
    MAX_RADIUS = 8

    def __init__(self, p=0.5, sigma=(0.1, 2, 0), extra_keys=None):
        if not 0 < sigma[0] <= sigma[1] or int(2.0 * sigma[1] + 0.5) > self.MAX_RADIUS:
            raise ValueError(f"GSGaussianBlurVoxelOpc: sigma range {tuple(sigma[:2])} must be positive and stay below 4.25 "
                             f"(the kernel gathers at most r = int(2 sigma + 0.5) = {self.MAX_RADIUS} cells)")
        self.p, self.sigma = p, sigma
        self.extra_keys = () if extra_keys is None else tuple(extra_keys)

    def draw(self, rng, data_dict):
        if not rng.random() < self.p:
            return dict(fired=False, sigma=None)
        return dict(fired=True, sigma=float(rng.uniform(self.sigma[0], self.sigma[1])))

    def apply(self, data_dict, params):
        if not params["fired"]:
            return data_dict
        if "grid_coord" not in data_dict:
            raise AssertionError(f"grid_coord is required for GSGaussianBlur, but only {list(data_dict.keys())} is provided")
        gc = data_dict["grid_coord"]
        if not isinstance(gc, torch.Tensor) or not gc.is_cuda:
            raise RuntimeError("GSGaussianBlurVoxelOpc: GPU tensors required (no CPU fallback)")
        if gc.dtype != torch.int32 or not gc.is_contiguous():
            gc = gc.to(torch.int32).contiguous()
        opacity = _dev(data_dict["opacity"], "opacity")
        mask = (opacity > 0.5).reshape(-1)
        extra = {k: _dev(data_dict[k], k) for k in self.KEYS if k in self.extra_keys}
        nv.voxel_blur_(gc, mask, _dev(data_dict["color"], "color", 3), params["sigma"], normalize_quat="quat" in extra, **extra)
        return data_dict


@TRANSFORMS.register_module()
class ContrastiveViewsGenerator_SSL(Transform):
    """transform.py:259-315: from clones of `view_keys`, two global views (global_base_transform, then global_transform0 /
    global_transform1 on a clone each) and local_crop_num local views (local_base_transform, then local_transform on a clone
    each) -> global_crop{0,1}_<key> and local_crop{i}_<key> for every key a view ends with; every other entry of data_dict stays.
    The five sub-lists are Compose objects of this module (they fuse like their parent).  draw() hands over a seed; the generators
    of the sub-list runs are spawned from it in the order global_base, local_base, global0, global1, local[0], local[1], ...;
    params["views"] replays one recorded params list per run in that same order."""

    def __init__(self, view_keys=("coord", "color", "normal", "origin_coord"), global_base_transform=None, local_base_transform=None,
                 global_transform0=None, global_transform1=None, local_transform=None, local_crop_num=4):
        self.view_keys = view_keys
        self.global_base_transform = Compose(global_base_transform)
        self.local_base_transform = Compose(local_base_transform)
        self.global_transform0 = Compose(global_transform0)
        self.global_transform1 = Compose(global_transform1)
        self.local_transform = Compose(local_transform)
        self.local_crop_num = local_crop_num

    def set_fuse(self, fuse):
        for c in (self.global_base_transform, self.local_base_transform, self.global_transform0, self.global_transform1,
                  self.local_transform):
            c.set_fuse(fuse)

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def _clone(self, d):
        return {k: (d[k].clone() if isinstance(d[k], torch.Tensor) else copy.deepcopy(d[k])) for k in self.view_keys}

    def apply(self, data_dict, params):
        runs = 4 + self.local_crop_num
        views = params.get("views")
        if views is not None and len(views) != runs:
            raise ValueError(f"ContrastiveViewsGenerator_SSL: {runs} params lists expected, got {len(views)}")
        rngs = [None] * runs if views is not None else \
            [np.random.default_rng(s) for s in np.random.SeedSequence(int(params["seed"])).spawn(runs)]

        def run(compose, d, k):
            return compose(d, params=None if views is None else views[k], rng=rngs[k])
        global_base = run(self.global_base_transform, self._clone(data_dict), 0)
        global0 = run(self.global_transform0, self._clone(global_base), 2)
        global1 = run(self.global_transform1, self._clone(global_base), 3)
        local_base = run(self.local_base_transform, self._clone(data_dict), 1)
        local = [run(self.local_transform, self._clone(local_base), 4 + i) for i in range(self.local_crop_num)]
        for key, value in global0.items():
            data_dict["global_crop0_" + key] = value
        for key, value in global1.items():
            data_dict["global_crop1_" + key] = value
        for i, d in enumerate(local):
            for key, value in d.items():
                data_dict["local_crop{}_".format(i) + key] = value
        return data_dict


@TRANSFORMS.register_module()
class CollectContrast(Transform):
    """transform.py:20-56: every entry whose name starts with one of `keys_prefix`, one [n] offset tensor per entry of
    offset_keys_dict (n = rows of the named entry) and every `<name>_keys=(...)` as `<name>`, the float32 column concatenation."""

    def __init__(self, keys_prefix, offset_keys_dict=None, **kwargs):
        self.keys = keys_prefix
        self.offset_keys = dict(offset="coord") if offset_keys_dict is None else offset_keys_dict
        self.kwargs = kwargs

    def apply(self, data_dict, params):
        data = dict()
        for key in ([self.keys] if isinstance(self.keys, str) else self.keys):
            for key_i in data_dict.keys():
                if key_i.startswith(key):
                    data[key_i] = data_dict[key_i]
        for key, value in self.offset_keys.items():
            data[key] = torch.tensor([data_dict[value].shape[0]], device=data_dict[value].device)
        for name, keys in self.kwargs.items():
            assert isinstance(keys, (list, tuple))
            data[name.replace("_keys", "")] = torch.cat([data_dict[k].float() for k in keys], dim=1)
        return data


# ---- the alternatives the shipped lists carry commented out, and the rest of the reference's per-sample transforms ---------------
@TRANSFORMS.register_module()
class HueSaturationTranslation(Transform):
    """transform.py:1035-1100: hue shifted by hue_val = (u - 0.5) 2 hue_max, saturation scaled by 1 + (u' - 0.5) 2 saturation_max,
    through the reference's fp64 HSV round trip that truncates to whole colour values (ss_aug_hsv: one pass, in place).  No family:
    a pending colour pass is flushed first, so the op sees what the chromatic ops in front of it wrote."""

    def __init__(self, hue_max=0.5, saturation_max=0.2):
        self.hue_max, self.saturation_max = hue_max, saturation_max

    def draw(self, rng, data_dict):
        return dict(hue_val=float((rng.random() - 0.5) * 2 * self.hue_max),
                    sat_ratio=float(1 + (rng.random() - 0.5) * 2 * self.saturation_max))

    def apply(self, data_dict, params):
        if "color" in data_dict:
            nv.aug_hsv_(_dev(data_dict["color"], "color", 3), params["hue_val"], params["sat_ratio"])
        return data_dict


@TRANSFORMS.register_module()
class RandomColorDrop(Transform):
    """transform.py:1103-1117: with probability p, color *= color_augment."""

    def __init__(self, p=0.2, color_augment=0.0):
        self.p, self.color_augment = p, color_augment

    def draw(self, rng, data_dict):
        return dict(fired=bool(rng.random() < self.p))

    def apply(self, data_dict, params):
        if params["fired"] and "color" in data_dict:
            _dev(data_dict["color"], "color").mul_(self.color_augment)
        return data_dict

    def __repr__(self):
        return "RandomColorDrop(color_augment: {}, p: {})".format(self.color_augment, self.p)


@TRANSFORMS.register_module()
class NormalizeCoord(Transform):
    """transform.py:423-434: coord <- (coord - centroid) / m, m = the largest distance from the centroid, and scale <- scale / m.
    Folds into the pending affine: ss_aug_moments of the pending A x + b gives the centroid, a second call after the shift the
    largest squared norm (a 4-double readback each, fp64), and the division rides the run's ss_aug_gaussians pass.  pc_coord stays
    as it is, as in the reference."""
    family = "rigid"

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.shift(data_dict, -state.moments(data_dict)[:3])
            m2 = float(state.moments(data_dict)[3])
            if not m2 > 0.0:                                  # the reference divides by m = 0 here and fills coord with NaN
                raise ValueError("NormalizeCoord: every point lies on the centroid")
            state.scale(data_dict, 1.0 / np.sqrt(m2))


@TRANSFORMS.register_module()
class PositiveShift(Transform):
    """transform.py:437-443: coord -= its per-axis minimum (the bounding box of the pending affine); pc_coord stays as it is."""
    family = "rigid"

    def fold(self, state, data_dict, params):
        if "coord" in data_dict:
            state.shift(data_dict, -state.bbox(data_dict)[:3])


@TRANSFORMS.register_module()
class PointClip(Transform):
    """transform.py:482-494: coord clipped to point_cloud_range = (x0, y0, z0, x1, y1, z1)."""

    def __init__(self, point_cloud_range=(-80, -80, -3, 80, 80, 1)):
        self.point_cloud_range = point_cloud_range

    def apply(self, data_dict, params):
        if "coord" in data_dict:
            coord = _dev(data_dict["coord"], "coord", 3)
            coord.clamp_(coord.new_tensor([float(v) for v in self.point_cloud_range[:3]]),
                         coord.new_tensor([float(v) for v in self.point_cloud_range[3:]]))
        return data_dict


@TRANSFORMS.register_module()
class Add(Transform):
    """transform.py:402-412: data_dict[key] = value for every entry of keys_dict (host only)."""

    def __init__(self, keys_dict=None):
        self.keys_dict = dict() if keys_dict is None else keys_dict

    def apply(self, data_dict, params):
        for key, value in self.keys_dict.items():
            data_dict[key] = value
        return data_dict


def _row_keys(*extra):
    return DROPOUT_KEYS + tuple(k for k in extra if k not in DROPOUT_KEYS)


# The reference permutes coord / grid_coord / displacement / color / normal / segment / instance and masks the same without
# displacement: on a Gaussian sample that leaves quat / scale / opacity / lang_feat paired with other rows.  Every per-point key moves here.
SHUFFLE_KEYS = _row_keys("grid_coord", "displacement")
CROP_BOUNDARY_KEYS = _row_keys("grid_coord")


def _take_keys(data_dict, keys, idx):
    idx32 = idx.to(torch.int32).contiguous()
    for k in keys:
        v = data_dict.get(k)
        if isinstance(v, torch.Tensor):
            data_dict[k] = gt.take_rows(v, idx32)
    return data_dict


@TRANSFORMS.register_module()
class ShufflePoint(Transform):
    """transform.py:1551-1571: the rows in a random order (torch.randperm on a seeded device generator, as RandomDropout draws);
    params["idx"] replays a recorded permutation.  Moves SHUFFLE_KEYS."""

    def draw(self, rng, data_dict):
        return dict(seed=_seed(rng))

    def apply(self, data_dict, params):
        assert "coord" in data_dict
        coord = data_dict["coord"]
        if not isinstance(coord, torch.Tensor) or not coord.is_cuda:
            raise RuntimeError("ShufflePoint: GPU tensors required (no CPU fallback)")
        n = coord.shape[0]
        if params.get("idx") is not None:
            idx = torch.as_tensor(np.asarray(params["idx"]), dtype=torch.int64).to(coord.device)
            if idx.shape != (n,):
                raise ValueError(f"ShufflePoint: a recorded permutation of {tuple(idx.shape)} for {n} rows")
        else:
            g = torch.Generator(device=coord.device)
            g.manual_seed(int(params["seed"]))
            idx = torch.randperm(n, device=coord.device, generator=g)
        return _take_keys(data_dict, SHUFFLE_KEYS, idx)


@TRANSFORMS.register_module()
class CropBoundary(Transform):
    """transform.py:1574-1592: the rows whose segment is neither 0 nor 1, in order.  Moves CROP_BOUNDARY_KEYS."""

    def apply(self, data_dict, params):
        assert "segment" in data_dict
        segment = data_dict["segment"]
        if not isinstance(segment, torch.Tensor) or not segment.is_cuda:
            raise RuntimeError("CropBoundary: GPU tensors required (no CPU fallback)")
        segment = segment.reshape(-1)
        return _take_keys(data_dict, CROP_BOUNDARY_KEYS, torch.nonzero((segment != 0) & (segment != 1)).reshape(-1))


@TRANSFORMS.register_module()
class ContrastiveViewsGenerator(Transform):
    """transform.py:1595-1617: two clones of `view_keys`, view_trans_cfg (a Compose of this module: it fuses like its parent) run
    on each -> view1_<key> / view2_<key> for every key a view ends with.  Both runs draw from the caller's Generator, one after
    the other, as the reference's two runs share the global stream: draw() hands it over; params["views"] = [params list of run
    1, of run 2] replays a recorded call instead."""

    def __init__(self, view_keys=("coord", "color", "normal", "origin_coord"), view_trans_cfg=None):
        self.view_keys = view_keys
        self.view_trans = Compose(view_trans_cfg)

    def set_fuse(self, fuse):
        self.view_trans.set_fuse(fuse)

    def draw(self, rng, data_dict):
        return dict(rng=rng)

    def _clone(self, d):
        return {k: (d[k].clone() if isinstance(d[k], torch.Tensor) else copy.deepcopy(d[k])) for k in self.view_keys}

    def apply(self, data_dict, params):
        views = params.get("views")
        if views is not None and len(views) != 2:
            raise ValueError(f"ContrastiveViewsGenerator: 2 params lists expected, got {len(views)}")
        view1, view2 = self._clone(data_dict), self._clone(data_dict)
        view1 = self.view_trans(view1, params=None if views is None else views[0], rng=params.get("rng"))
        view2 = self.view_trans(view2, params=None if views is None else views[1], rng=params.get("rng"))
        for key, value in view1.items():
            data_dict["view1_" + key] = value
        for key, value in view2.items():
            data_dict["view2_" + key] = value
        return data_dict


@TRANSFORMS.register_module()
class InstanceParser(Transform):
    """transform.py:1620-1664: rows whose segment is in segment_ignore_index get instance_ignore_index; the ids of the others
    become dense (0 .. K-1 in ascending order of the raw id -- signed: an id of -1 on a valid segment is an instance of its own,
    as np.unique makes it); `instance` is rewritten in place, `instance_centroid` (n, 3) holds each row's instance centroid and
    `bbox` (K, 8) = {centre, size, 0, class} with the class index shifted down past the non-negative ignore indices.  Both are
    fp32 (the reference: fp64 arrays of fp32 values).  The ids are ordered by the stable radix argsort with the ignored rows keyed
    past every id, ss_pool_partition turns the order into the CSR, ss_instance_boxes / ss_instance_scatter do the rest; two small
    readbacks (the id range, K)."""

    def __init__(self, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1):
        self.segment_ignore_index = segment_ignore_index
        self.instance_ignore_index = instance_ignore_index

    def apply(self, data_dict, params):
        coord = _dev(data_dict["coord"], "coord", 3)
        segment, instance = data_dict["segment"], data_dict["instance"]
        for t, name in ((segment, "segment"), (instance, "instance")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{name}: scenesplat_amd transforms need a GPU tensor (no CPU fallback)")
        n = coord.shape[0]
        if instance.shape != (n,) or instance.dtype not in (torch.int32, torch.int64) or not instance.is_contiguous():
            raise RuntimeError(f"instance: must be a contiguous (n,) int32 / int64 tensor (it is updated in place), got "
                               f"{tuple(instance.shape)} {instance.dtype}")
        segment = segment.reshape(-1).to(torch.int64).contiguous()
        if segment.shape[0] != n:
            raise RuntimeError(f"segment: {segment.shape[0]} rows, coord has {n}")
        ignore = [int(v) for v in self.segment_ignore_index]
        K, cluster, order, idx_ptr = 0, None, None, None
        if n > 0:
            valid = ~torch.isin(segment, torch.tensor(ignore, dtype=torch.int64, device=coord.device)) if ignore else \
                torch.ones(n, dtype=torch.bool, device=coord.device)
            ids = instance.to(torch.int64)
            big = torch.iinfo(torch.int64).max
            lo, hi, count = torch.stack([torch.where(valid, ids, big).min(), torch.where(valid, ids, -big).max(), valid.sum()]).tolist()
            if count > 0:
                span = hi - lo
                if span >= (1 << 62):
                    raise ValueError("InstanceParser: instance ids span more than 2^62")
                key = torch.where(valid, ids - lo, span + 1).contiguous()
                order, _, _ = nv.argsort_i64(key[None], (span + 1).bit_length(), want_inverse=False, want_sorted=False)
                order = order[0]
                cluster, idx_ptr, _, n_out = nv.pool_partition(key, order, 0)
                K = int(n_out.item()) - (1 if count < n else 0)
        bbox, centroid = nv.instance_boxes(coord, segment, order, idx_ptr, K, [v for v in ignore if v >= 0]) if K > 0 else \
            (torch.empty((0, 8), dtype=torch.float32, device=coord.device), None)
        data_dict["instance_centroid"] = nv.instance_scatter_(instance, cluster, K, centroid, self.instance_ignore_index)
        data_dict["bbox"] = bbox
        return data_dict


class Compose:
    """The reference's Compose (transform.py:1667-1677) with a seedable host Generator for every draw and, with fuse=True, runs of
    rigid ops and of colour ops folded into one kernel pass each (module docstring).  `params` replays one recorded dict per op."""

    def __init__(self, cfg=None, fuse=True, seed=None):
        self.cfg = cfg if cfg is not None else []
        self.transforms = [TRANSFORMS.build(c) if isinstance(c, dict) else c for c in self.cfg]
        self.rng = np.random.default_rng(seed)
        self.set_fuse(fuse)

    def set_fuse(self, fuse):
        """fuse / do not fuse, here and in the sub-lists of a nested ContrastiveViewsGenerator_SSL"""
        self.fuse = fuse
        for t in self.transforms:
            if hasattr(t, "set_fuse"):
                t.set_fuse(fuse)

    def __call__(self, data_dict, params=None, rng=None):
        """rng: the Generator of this call's draws (a nested list is handed one per run); default: the list's own."""
        if params is not None and len(params) != len(self.transforms):
            raise ValueError("Compose: one params dict per transform")
        rng = self.rng if rng is None else rng
        state = None
        for i, t in enumerate(self.transforms):
            p = params[i] if params is not None else t.draw(rng, data_dict)
            fam = t.family if self.fuse else None
            if state is not None and state.family != fam:
                state.flush(data_dict)
                state = None
            if fam is None:
                data_dict = t.apply(data_dict, p)
            else:
                if state is None:
                    state = _STATES[fam]()
                t.fold(state, data_dict, p)
        if state is not None:
            state.flush(data_dict)
        return data_dict
