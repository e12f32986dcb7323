"""torch-ngp's `raymarching` operator module (raymarching/raymarching.py) on the HIP path (csrc/raymarch.hip): the same function names and argument orders, so that
nerf/renderer.py:714, 737, 767, 802 and 822 run against it after one changed import line.  fp32 throughout, as the reference's wrappers cast.

Differences from the reference, all deliberate (DESIGN.md sections 5.13 and 8):
  * the arithmetic is fixed — no contraction, IEEE division, mrf_exp where the reference has __expf — so tests/raymarch_refs.py restates every operator bit for bit;
  * march_rays_train's point offsets rays[:, 0] are the exclusive prefix sum of the per-ray counts in ray order, the same in every run (the reference hands them out
    with an atomic counter, in arrival order; its consumers accept any order);
  * every marching loop terminates: a ray with a zero or non-finite direction or a NaN near / far takes no step, and the voxel-skipping loop also ends at t >= far
    and when t stops advancing;
  * march_rays_train and march_rays take `noises=` (f32 [N] / [n_alive]) in addition; with perturb and no noises they draw torch.rand on the device as the reference does;
  * sph_from_ray is present and raises: nothing in the reference calls it.
"""
import torch
from torch.autograd import Function

from ._lib import lib, check, ptr, stream_ptr

__all__ = ["near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "flatten_rays", "march_rays_train", "composite_rays_train", "march_rays",
           "composite_rays"]

MAX_CASCADES = 8


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("raymarching: no GPU visible to torch (the operators run on the device only)")
    return torch.device("cuda")


def _f32(x, name, shape=None):
    """Checks x (a floating tensor of `shape`) without touching the device; _up moves it afterwards, so bad arguments are refused on any machine."""
    if not torch.is_tensor(x):
        raise TypeError("%s: a tensor expected, got %s" % (name, type(x).__name__))
    if not x.is_floating_point():
        raise TypeError("%s: a floating tensor expected, got %s" % (name, x.dtype))
    if shape is not None:
        _shaped(x, name, shape)
    return x


def _rays3(x, name):
    x = _f32(x, name)
    if x.numel() % 3:
        raise ValueError("%s: shape %s is no list of 3-vectors" % (name, tuple(x.shape)))
    return x.reshape(-1, 3)


def _up(x):
    """A contiguous fp32 device copy (the reference: custom_fwd(cast_inputs=torch.float32), .cuda(), .contiguous())."""
    return x.detach().to(_dev(), torch.float32).contiguous()


def _shaped(x, name, shape):
    if x.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(x.shape, shape)):
        raise ValueError("%s: shape %s, expected %s" % (name, tuple(x.shape), tuple("*" if s is None else s for s in shape)))
    return x


def _i32(x, name, shape):
    if not torch.is_tensor(x) or x.dtype != torch.int32:
        raise TypeError("%s: an int32 tensor expected, got %s" % (name, x.dtype if torch.is_tensor(x) else type(x).__name__))
    return _shaped(x, name, shape)


def _inplace_f32(x, name, shape):
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise TypeError("%s: a float32 tensor expected, got %s" % (name, x.dtype if torch.is_tensor(x) else type(x).__name__))
    return _shaped(x, name, shape)


def _resident(x, name):
    """A tensor the kernels write in place (or whose copy would be wasted): it must already be on the device and contiguous."""
    if not x.is_cuda or not x.is_contiguous():
        raise ValueError("%s: a contiguous device tensor expected" % name)
    return x


def _grid_args(who, density_bitfield, C_, H):
    C_, H = int(C_), int(H)
    if C_ < 1 or C_ > MAX_CASCADES:
        raise ValueError("%s: %d cascades, expected 1 .. %d" % (who, C_, MAX_CASCADES))
    if H < 2 or H > 1024 or H & (H - 1):
        raise ValueError("%s: H = %d is not a power of two in [2, 1024]" % (who, H))
    if not torch.is_tensor(density_bitfield) or density_bitfield.dtype != torch.uint8:
        raise TypeError("%s: density_bitfield must be a uint8 tensor" % who)
    if density_bitfield.dim() != 1 or density_bitfield.numel() != C_ * H ** 3 // 8:
        raise ValueError("%s: density_bitfield of %s, expected [%d] (C * H^3 / 8)" % (who, tuple(density_bitfield.shape), C_ * H ** 3 // 8))
    return density_bitfield, C_, H


def _march_scalars(who, bound, dt_gamma, max_steps):
    bound, dt_gamma, max_steps = float(bound), float(dt_gamma), int(max_steps)
    if not (0 < bound < 3e38):
        raise ValueError("%s: bound %r" % (who, bound))
    if not (0 <= dt_gamma < 3e38):
        raise ValueError("%s: dt_gamma %r" % (who, dt_gamma))
    if max_steps < 1 or max_steps > 1 << 24:
        raise ValueError("%s: max_steps %r" % (who, max_steps))
    return bound, dt_gamma, max_steps


def _noises(who, noises, perturb, n, dev):
    if noises is not None:
        return _up(noises)
    if perturb:
        return torch.rand(n, dtype=torch.float32, device=dev)
    return torch.zeros(n, dtype=torch.float32, device=dev)


# ----------------------------------------
# utils
# ----------------------------------------

def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.2):
    """rays_o, rays_d [N, 3], aabb [6] (xmin, ymin, zmin, xmax, ymax, zmax) -> nears, fars f32 [N]; a ray that misses the box has both at FLT_MAX."""
    rays_o = _rays3(rays_o, "near_far_from_aabb: rays_o")
    rays_d = _rays3(rays_d, "near_far_from_aabb: rays_d")
    if rays_o.shape != rays_d.shape:
        raise ValueError("near_far_from_aabb: rays_o %s and rays_d %s differ" % (tuple(rays_o.shape), tuple(rays_d.shape)))
    aabb = _f32(aabb, "near_far_from_aabb: aabb", (6,))
    rays_o, rays_d, aabb = _up(rays_o), _up(rays_d), _up(aabb)
    N = rays_o.shape[0]
    nears = torch.empty(N, dtype=torch.float32, device=rays_o.device)
    fars = torch.empty(N, dtype=torch.float32, device=rays_o.device)
    check(lib().mirres_rm_near_far(ptr(rays_o), ptr(rays_d), ptr(aabb), N, float(min_near), ptr(nears), ptr(fars), stream_ptr()), "mirres_rm_near_far")
    return nears, fars


def sph_from_ray(rays_o, rays_d, radius):
    raise NotImplementedError("sph_from_ray: nothing in the reference calls it (raymarching/raymarching.py:52-80 has no user); not built")


def morton3D(coords):
    """coords int [N, 3] in [0, 1024) -> indices i32 [N]."""
    if not torch.is_tensor(coords) or coords.is_floating_point():
        raise TypeError("morton3D: an integer tensor expected")
    coords = _shaped(coords, "morton3D: coords", (None, 3)).to(_dev()).int().contiguous()
    N = coords.shape[0]
    indices = torch.empty(N, dtype=torch.int32, device=coords.device)
    check(lib().mirres_rm_morton3d(ptr(coords), N, ptr(indices), stream_ptr()), "mirres_rm_morton3d")
    return indices


def morton3D_invert(indices):
    """indices int [N] -> coords i32 [N, 3]."""
    if not torch.is_tensor(indices) or indices.is_floating_point():
        raise TypeError("morton3D_invert: an integer tensor expected")
    indices = _shaped(indices, "morton3D_invert: indices", (None,)).to(_dev()).int().contiguous()
    N = indices.shape[0]
    coords = torch.empty(N, 3, dtype=torch.int32, device=indices.device)
    check(lib().mirres_rm_morton3d_invert(ptr(indices), N, ptr(coords), stream_ptr()), "mirres_rm_morton3d_invert")
    return coords


def packbits(grid, thresh, bitfield=None):
    """grid f32 [C, H^3] (H^3 a multiple of 8), thresh -> bitfield u8 [C * H^3 / 8] (written in place when given): bit i of byte n = grid[8 n + i] > thresh."""
    grid = _f32(grid, "packbits: grid", (None, None))
    if grid.shape[1] % 8:
        raise ValueError("packbits: %d values per cascade is no multiple of 8" % grid.shape[1])
    N = grid.shape[0] * grid.shape[1] // 8
    if bitfield is not None and (not torch.is_tensor(bitfield) or bitfield.dtype != torch.uint8 or bitfield.numel() != N):
        raise ValueError("packbits: bitfield must be a uint8 tensor of %d bytes" % N)
    grid = _up(grid)
    if bitfield is None:
        bitfield = torch.empty(N, dtype=torch.uint8, device=grid.device)
    else:
        _resident(bitfield, "packbits: bitfield")
    check(lib().mirres_rm_packbits(ptr(grid), N, float(thresh), ptr(bitfield), stream_ptr()), "mirres_rm_packbits")
    return bitfield


def flatten_rays(rays, M):
    """rays i32 [N, 2] (offset, count), M -> res i32 [M]: the ray of every point.  A ray whose span leaves [0, M) writes nothing."""
    rays = _i32(rays, "flatten_rays: rays", (None, 2))
    M = int(M)
    if M < 0:
        raise ValueError("flatten_rays: M %d" % M)
    rays = rays.to(_dev()).contiguous()
    res = torch.zeros(M, dtype=torch.int32, device=rays.device)
    check(lib().mirres_rm_flatten_rays(ptr(rays), rays.shape[0], M, ptr(res) if M else None, stream_ptr()), "mirres_rm_flatten_rays")
    return res


# ----------------------------------------
# train functions
# ----------------------------------------

def march_rays_train(rays_o, rays_d, bound, contract, density_bitfield, C, H, nears, fars, perturb=False, dt_gamma=0, max_steps=1024, noises=None):
    """-> xyzs f32 [M, 3], dirs f32 [M, 3], ts f32 [M, 2] (t after the step, dt), rays i32 [N, 2] (offset, count): the points of ray i are
    xyzs[rays[i, 0] : rays[i, 0] + rays[i, 1]], and rays[:, 0] is the exclusive prefix sum of rays[:, 1]."""
    who = "march_rays_train"
    rays_o = _rays3(rays_o, who + ": rays_o")
    rays_d = _rays3(rays_d, who + ": rays_d")
    if rays_o.shape != rays_d.shape:
        raise ValueError("%s: rays_o %s and rays_d %s differ" % (who, tuple(rays_o.shape), tuple(rays_d.shape)))
    bits, C_, H = _grid_args(who, density_bitfield, C, H)
    bound, dt_gamma, max_steps = _march_scalars(who, bound, dt_gamma, max_steps)
    N = rays_o.shape[0]
    nears = _f32(nears, who + ": nears", (N,))
    fars = _f32(fars, who + ": fars", (N,))
    if noises is not None:
        _f32(noises, who + ": noises", (N,))
    rays_o, rays_d, nears, fars, bits = _up(rays_o), _up(rays_d), _up(nears), _up(fars), bits.to(_dev()).contiguous()
    dev = rays_o.device
    noises = _noises(who, noises, perturb, N, dev)
    rays = torch.empty(N, 2, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    L, s = lib(), stream_ptr()
    head = (ptr(rays_o), ptr(rays_d), ptr(bits), bound, int(bool(contract)), dt_gamma, max_steps, N, C_, H, ptr(nears), ptr(fars), ptr(noises))
    check(L.mirres_rm_march_train_count(*head, ptr(rays), s), "mirres_rm_march_train_count")
    check(L.mirres_rm_march_train_scan(ptr(rays), N, ptr(total), s), "mirres_rm_march_train_scan")
    M = int(total.item())
    if M > 2 ** 31 - 1:
        raise ValueError("%s: %d points do not fit the int32 offsets of `rays`: march fewer rays at a time" % (who, M))
    xyzs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    dirs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    ts = torch.zeros(M, 2, dtype=torch.float32, device=dev)
    if M:
        check(L.mirres_rm_march_train_write(*head, ptr(rays), M, ptr(xyzs), ptr(dirs), ptr(ts), s), "mirres_rm_march_train_write")
    return xyzs, dirs, ts, rays


class _composite_rays_train(Function):
    @staticmethod
    def forward(ctx, sigmas, rgbs, ts, rays, T_thresh, alpha_mode):
        # composite_rays_train below has checked the arguments and brought them to the device in fp32
        sigmas, rgbs = sigmas.contiguous(), rgbs.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        dev = sigmas.device
        weights = torch.zeros(M, dtype=torch.float32, device=dev)            # may be left unmodified behind an early stop
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty(N, 3, dtype=torch.float32, device=dev)
        T_thresh, alpha_mode = float(T_thresh), int(bool(alpha_mode))
        nz = lambda t: ptr(t) if M else None
        check(lib().mirres_rm_composite_train_fwd(nz(sigmas), nz(rgbs), nz(ts), ptr(rays), M, N, T_thresh, alpha_mode, nz(weights), ptr(weights_sum) if N else None,
                                                  ptr(depth) if N else None, ptr(image) if N else None, stream_ptr()), "mirres_rm_composite_train_fwd")
        ctx.save_for_backward(sigmas, rgbs, ts, rays, weights_sum, depth, image)
        ctx.dims = [M, N, T_thresh, alpha_mode]
        return weights, weights_sum, depth, image

    @staticmethod
    def backward(ctx, grad_weights, grad_weights_sum, grad_depth, grad_image):
        sigmas, rgbs, ts, rays, weights_sum, depth, image = ctx.saved_tensors
        M, N, T_thresh, alpha_mode = ctx.dims
        g = [x.to(torch.float32).contiguous() for x in (grad_weights, grad_weights_sum, grad_depth, grad_image)]
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        if M and N:
            check(lib().mirres_rm_composite_train_bwd(ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(sigmas), ptr(rgbs), ptr(ts), ptr(rays), ptr(weights_sum), ptr(depth),
                                                      ptr(image), M, N, T_thresh, alpha_mode, ptr(grad_sigmas), ptr(grad_rgbs), stream_ptr()),
                  "mirres_rm_composite_train_bwd")
        return grad_sigmas, grad_rgbs, None, None, None, None


def composite_rays_train(sigmas, rgbs, ts, rays, T_thresh=1e-4, alpha_mode=False):
    """sigmas [M], rgbs [M, 3], ts [M, 2], rays i32 [N, 2] -> weights [M], weights_sum [N], depth [N], image [N, 3] (premultiplied).  Differentiable in sigmas and rgbs;
    the cast to fp32 and the move to the device happen here, outside the Function (the reference: custom_fwd(cast_inputs=torch.float32)), so a half or host tensor
    receives its gradient in its own dtype and place."""
    who = "composite_rays_train"
    sigmas = _f32(sigmas, who + ": sigmas", (None,))
    M = sigmas.shape[0]
    rgbs = _f32(rgbs, who + ": rgbs", (M, 3))
    ts = _f32(ts, who + ": ts", (M, 2))
    rays = _i32(rays, who + ": rays", (None, 2))
    dev = _dev()
    return _composite_rays_train.apply(sigmas.to(dev, torch.float32), rgbs.to(dev, torch.float32), _up(ts), rays.to(dev).contiguous(), T_thresh, alpha_mode)


# ----------------------------------------
# infer functions
# ----------------------------------------

def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, contract, density_bitfield, C, H, near, far, perturb=False, dt_gamma=0, max_steps=1024,
               noises=None):
    """March the first n_alive rays named by rays_alive for at most n_step samples each, from rays_t -> xyzs, dirs f32 [n_alive * n_step, 3], ts f32 [n_alive * n_step, 2];
    slots a ray did not fill stay zero."""
    who = "march_rays"
    rays_o = _rays3(rays_o, who + ": rays_o")
    rays_d = _rays3(rays_d, who + ": rays_d")
    if rays_o.shape != rays_d.shape:
        raise ValueError("%s: rays_o %s and rays_d %s differ" % (who, tuple(rays_o.shape), tuple(rays_d.shape)))
    bits, C_, H = _grid_args(who, density_bitfield, C, H)
    bound, dt_gamma, max_steps = _march_scalars(who, bound, dt_gamma, max_steps)
    N = rays_o.shape[0]
    n_alive, n_step = int(n_alive), int(n_step)
    if n_step < 1 or n_step > 65536:
        raise ValueError("%s: n_step %d" % (who, n_step))
    rays_alive = _i32(rays_alive, who + ": rays_alive", (None,))
    if n_alive < 0 or n_alive > rays_alive.shape[0]:
        raise ValueError("%s: n_alive %d, rays_alive has %d entries" % (who, n_alive, rays_alive.shape[0]))
    rays_t = _f32(rays_t, who + ": rays_t", (N,))
    near = _f32(near, who + ": near", (N,))
    far = _f32(far, who + ": far", (N,))
    if noises is not None:
        _f32(noises, who + ": noises", (n_alive,))
    rays_o, rays_d, rays_t, near, far, bits = _up(rays_o), _up(rays_d), _up(rays_t), _up(near), _up(far), bits.to(_dev()).contiguous()
    rays_alive = rays_alive.to(_dev()).contiguous()
    dev = rays_o.device
    M = n_alive * n_step
    xyzs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    dirs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
    ts = torch.zeros(M, 2, dtype=torch.float32, device=dev)
    noises = _noises(who, noises, perturb, n_alive, dev)
    if M:
        check(lib().mirres_rm_march(n_alive, n_step, ptr(rays_alive), ptr(rays_t), ptr(rays_o), ptr(rays_d), N, bound, int(bool(contract)), dt_gamma, max_steps, C_, H,
                                    ptr(bits), ptr(near), ptr(far), ptr(xyzs), ptr(dirs), ptr(ts), ptr(noises), stream_ptr()), "mirres_rm_march")
    return xyzs, dirs, ts


def composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh=1e-2, alpha_mode=False):
    """Accumulate n_step samples of the first n_alive rays into weights_sum, depth [N] and image [N, 3] IN PLACE; a ray that ends (opacity, or a slot the marcher left
    empty) gets rays_alive = -1, every other ray its new rays_t."""
    who = "composite_rays"
    n_alive, n_step = int(n_alive), int(n_step)
    if n_step < 1 or n_step > 65536:
        raise ValueError("%s: n_step %d" % (who, n_step))
    rays_alive = _i32(rays_alive, who + ": rays_alive", (None,))
    if n_alive < 0 or n_alive > rays_alive.shape[0]:
        raise ValueError("%s: n_alive %d, rays_alive has %d entries" % (who, n_alive, rays_alive.shape[0]))
    weights_sum = _inplace_f32(weights_sum, who + ": weights_sum", (None,))
    N = weights_sum.shape[0]
    rays_t = _inplace_f32(rays_t, who + ": rays_t", (N,))
    depth = _inplace_f32(depth, who + ": depth", (N,))
    image = _inplace_f32(image, who + ": image", (N, 3))
    M = n_alive * n_step
    sigmas = _f32(sigmas, who + ": sigmas", (M,))
    rgbs = _f32(rgbs, who + ": rgbs", (M, 3))
    ts = _f32(ts, who + ": ts", (M, 2))
    for t, nm in ((rays_alive, "rays_alive"), (rays_t, "rays_t"), (weights_sum, "weights_sum"), (depth, "depth"), (image, "image")):
        _resident(t, who + ": " + nm)
    sigmas, rgbs, ts = _up(sigmas), _up(rgbs), _up(ts)
    if M:
        check(lib().mirres_rm_composite(n_alive, n_step, N, float(T_thresh), int(bool(alpha_mode)), ptr(rays_alive), ptr(rays_t), ptr(sigmas), ptr(rgbs), ptr(ts),
                                        ptr(weights_sum), ptr(depth), ptr(image), stream_ptr()), "mirres_rm_composite")
    return tuple()
