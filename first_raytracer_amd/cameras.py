"""Cameras for Context.radiance_rays / Context.render_camera: numpy, no device.

Each returns (ny * nx, 8) float32 ray records (frt.h frtx_radiance_rays: origin, t_max,
direction, RNG stream id) in row-major texel order, row 0 first, with streams arange and
t_max = FLT_MAX.  jitter: where in its texel a ray passes -- None: the centre (0.5, 0.5); a
(2,) pair (jx, jy) in [0, 1)^2 for every texel (render_camera's passes); or an (ny, nx, 2)
array of pairs.

latlong follows the environment image's convention (frt_set_env_image: phi = atan2(d.x, -d.z),
theta = acos(d.y), u = phi / 2 pi, v = theta / pi, row 0 = the +y pole), so an image rendered
with it, reshaped to (ny, nx, 3), can be handed back as an environment image as it is.
"""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def _texel_uv(nx, ny, jitter):
    """(u, v) in [0, 1)^2 per texel, (ny, nx) each: u across a row, v down the rows."""
    if jitter is None:
        jx = jy = 0.5
    else:
        j = np.asarray(jitter, np.float64)
        if j.shape == (2,):
            jx, jy = j
        elif j.shape == (ny, nx, 2):
            jx, jy = j[..., 0], j[..., 1]
        else:
            raise ValueError(f"jitter: a (2,) pair or an ({ny}, {nx}, 2) array, not {j.shape}")
        if np.any(j < 0) or np.any(j >= 1):
            raise ValueError("jitter: values in [0, 1)")
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return (x + jx) / nx, (y + jy) / ny


def _records(origins, directions):
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origins, np.float64).reshape(-1, 3), d.shape)
    rec = np.zeros((len(d), 8), np.float32)
    rec[:, 0:3] = o
    rec[:, 3] = FLT_MAX
    rec[:, 4:7] = d
    rec.view(np.uint32)[:, 7] = np.arange(len(d), dtype=np.uint32)
    return rec


def _frame(forward, up):
    w = np.asarray(forward, np.float64)
    w = w / np.linalg.norm(w)
    u = np.cross(w, np.asarray(up, np.float64))
    if np.linalg.norm(u) < 1e-12:
        raise ValueError("up is parallel to forward")
    u = u / np.linalg.norm(u)          # right
    return u, np.cross(u, w), w        # right, true up, forward


def latlong_directions(nx, ny, jitter=None):
    """Unit directions (ny, nx, 3) of the lat-long texels (the module's convention)."""
    u, v = _texel_uv(nx, ny, jitter)
    phi, theta = 2.0 * np.pi * u, np.pi * v
    st = np.sin(theta)
    return np.stack([st * np.sin(phi), np.cos(theta), -st * np.cos(phi)], axis=-1)


def latlong_solid_angles(nx, ny):
    """Solid angle (ny, nx) of each lat-long texel: (2 pi / nx) (cos theta_top - cos theta_bottom)."""
    edges = np.cos(np.pi * np.arange(ny + 1, dtype=np.float64) / ny)
    return np.repeat(((edges[:-1] - edges[1:]) * (2.0 * np.pi / nx))[:, None], nx, axis=1)


def latlong(origin, nx, ny, jitter=None):
    """Every direction around `origin`: a light probe, nx x ny texels (nx = 2 ny keeps them square)."""
    return _records(origin, latlong_directions(nx, ny, jitter))


def orthographic(origin, forward, up, width, height, nx, ny, jitter=None):
    """Parallel rays along `forward` from a width x height rectangle centred at `origin`; row 0
    is the top edge (towards `up`), column 0 the left one."""
    right, true_up, w = _frame(forward, up)
    u, v = _texel_uv(nx, ny, jitter)
    o = (np.asarray(origin, np.float64) + ((u - 0.5) * width)[..., None] * right +
         ((0.5 - v) * height)[..., None] * true_up)
    return _records(o, np.broadcast_to(w, o.shape))


def fisheye(origin, forward, up, fov_deg, nx, ny, jitter=None):
    """Equidistant fisheye: the angle from `forward` grows linearly with the distance from the
    image centre and reaches fov_deg / 2 on the circle inscribed in the frame.  Returns
    (records, outside): outside (ny * nx,) bool marks the texels beyond that circle; their
    records point along `forward` (valid rays; mask their results out)."""
    if not 0.0 < fov_deg <= 360.0:
        raise ValueError("fov_deg in (0, 360]")
    right, true_up, w = _frame(forward, up)
    u, v = _texel_uv(nx, ny, jitter)
    # centred coordinates in units of the inscribed circle's radius
    half = 0.5 * min(nx, ny)
    x, y = (u - 0.5) * nx / half, (0.5 - v) * ny / half
    r = np.sqrt(x * x + y * y)
    outside = r > 1.0
    ang = r * np.radians(fov_deg) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        cx, cy = np.where(r > 0, x / r, 0.0), np.where(r > 0, y / r, 0.0)
    s = np.sin(ang)
    d = (s * cx)[..., None] * right + (s * cy)[..., None] * true_up + np.cos(ang)[..., None] * w
    d[outside] = w
    return _records(origin, d), outside.reshape(-1)
