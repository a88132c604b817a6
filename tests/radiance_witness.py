"""The numpy witness of the radiance arithmetic the frame kernels share: the sky and sun models (headers/sky.glsl:1-113), the albedo
modulation (headers/color.glsl:1-31, final_gather.rchit:68-80) and the spatial hash's keys and insert (headers/spatial_hash.glsl:105-195).
A helper module, not a test: tests/test_radiance_witness.py holds the C oracle to it on the CPU, tests/test_gpu_radiance_functions.py the
device functions (dust_hip_device_eval 15..19). Written from the shader text; binds neither library and shares no code with oracle/ or csrc/.

Evaluation is float64 with the shaders' float32 literals widened -- except the ill-conditioned front ends, which are numpy float32
operation by operation in the shader's order (every side builds with contraction off, so these are the same IEEE operations):
  sky: cos_gamma = (dx*sx + dy*sy) + dz*sz   (acos has unbounded condition at 1: a float64 dot product misses by 1e-3 next to the sun)
  sun: the same cos_gamma, singamma = 1 - cos_gamma*cos_gamma, ar2 = 1 / (sinf(R)*sinf(R)), sc2 = 1 - (ar2*singamma)*singamma
Where the float32 cos_gamma leaves [-1, 1] the sky is NaN in all three channels (acos of it is, on every side).
The integer parts (pcg, xxhash32, fingerprint, location, the insert's control flow) are exact.

LogLuv fields of an insert: the witness encodes in float64 and FLAGS a row whose log-luminance lies within 4e-3 of a quantisation step,
or a chroma within 1e-3 of one; a float32 implementation may land on the other side there and nowhere else. Where the figures come from
(in steps): float32 log2(Y) + 20 lies in [0, 40), so a 1-ulp log2 and the rounding of the sum are <= 2e-6 + 1.9e-6, times 409.6 = 1.6e-3;
the product's own rounding below 16384 adds 5e-4; a merge adds the decoded value's error, (Le + 0.5) / 409.6 - 20 rounded twice below 32
and a 1-ulp exp2, 1.5e-6 relative, which is 9e-4: 3e-3 in all. Chroma: 820 u <= 511 with u off by a dozen float32 roundings (1e-6) is 5e-4."""
import numpy as np

F = np.float32
U32 = 0xFFFFFFFF
L_STEP_GUARD, UV_STEP_GUARD = 4e-3, 1e-3

# GLSL mat3 constructors list COLUMNS; row i of the arrays below is output component i
XYZ_TO_ACESCG = np.array([[1.6410228, -0.32480323, -0.23642465], [-0.66366285, 1.6153315, 0.016756356],
                          [0.011721907, -0.0082844375, 0.9883947]], F).astype(np.float64)
ACESCG_TO_XYZ = np.array([[0.66245437, 0.13400422, 0.15618773], [0.2722288, 0.6740818, 0.05368953],
                          [-0.0055746622, 0.00406073, 1.0103393]], F).astype(np.float64)
SRGB_TO_ACESCG = np.array([[0.6031065, 0.32633433, 0.047995567], [0.07011794, 0.9199162, 0.012763573],
                           [0.022178888, 0.11607823, 0.94101846]], F).astype(np.float64)
ACESCG_TO_SRGB = np.array([[1.7312546, -0.6040432, -0.08010775], [-0.131619, 1.1348418, -0.008679431],
                           [-0.024568284, -0.12575036, 1.0656371]], F).astype(np.float64)


# ------------------------------------------------------------------ sky.glsl
def cos_gamma32(state, dirs):
    s, d = np.asarray(state, F), np.asarray(dirs, F)
    with np.errstate(all="ignore"):
        return ((d[:, 0] * s[48]).astype(F) + (d[:, 1] * s[49]).astype(F)).astype(F) + (d[:, 2] * s[50]).astype(F)


def sky_radiance(state, dirs):
    """(n, 3) float64. state: the 56 floats (per channel 9 configuration values, radiance, 6 darkening coefficients; then the sun's
    direction, one pad, the solar intensity and the solar radius)."""
    s64 = np.asarray(state, F).astype(np.float64)
    d = np.asarray(dirs, F)
    if s64[49] <= 0:
        return np.zeros((len(d), 3))
    cg32 = cos_gamma32(state, d)
    bad = ~(np.abs(cg32) <= 1)
    cg = np.where(bad, 0.0, cg32.astype(np.float64))
    cos_theta = np.clip(d[:, 1].astype(np.float64), 0.0, 1.0)
    gamma = np.arccos(cg)
    xyz = np.empty((len(d), 3))
    for k in range(3):
        c = s64[16 * k: 16 * k + 9]
        exp_m = np.exp(c[4] * gamma)
        ray_m = cg * cg
        mie_m = (1.0 + ray_m) / np.power(1.0 + c[8] * c[8] - 2.0 * c[8] * cg, 1.5)
        zenith = np.sqrt(cos_theta)
        v = (1.0 + c[0] * np.exp(c[1] / (cos_theta + float(F(0.01))))) * (c[2] + c[3] * exp_m + c[5] * ray_m + c[6] * mie_m + c[7] * zenith)
        xyz[:, k] = v * s64[16 * k + 9] * 683.0
    rgb = xyz @ XYZ_TO_ACESCG.T
    rgb[bad] = np.nan
    return rgb


def sun_sc2(state, dirs):
    """the float32 front end of the sun: sc2 per direction, whatever the early-outs decide"""
    s = np.asarray(state, F)
    cg = cos_gamma32(state, dirs)
    with np.errstate(all="ignore"):
        sol = F(np.sin(np.float64(s[55])))  # sinf, correctly rounded
        ar2 = F(1.0) / (sol * sol).astype(F)
        singamma = F(1.0) - (cg * cg).astype(F)
        return (F(1.0) - ((ar2 * singamma).astype(F) * singamma).astype(F)).astype(F)


def _darkened(s64, sc):
    xyz = np.empty((len(sc), 3))
    for k in range(3):
        ld = s64[16 * k + 10: 16 * k + 16]
        xyz[:, k] = s64[52 + k] * sum(ld[j] * sc ** j for j in range(6))
    return xyz @ XYZ_TO_ACESCG.T


def sun_radiance(state, dirs):
    """((n, 3) float64, sc2 float32)"""
    s64 = np.asarray(state, F).astype(np.float64)
    d = np.asarray(dirs, F)
    cg, sc2 = cos_gamma32(state, d), sun_sc2(state, d)
    dark = ~((cg < 0) | (d[:, 1] < 0) | (sc2 <= 0))
    rgb = _darkened(s64, np.sqrt(np.where(dark, sc2.astype(np.float64), 0.0)))
    rgb[~dark] = 0.0
    return rgb, sc2


def sun_centre(state):
    """the disk's centre: sampleCosine 1"""
    return _darkened(np.asarray(state, F).astype(np.float64), np.ones(1))[0]


def normalize32(d):
    d = np.asarray(d, np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    n = np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
    return (d / n[:, None]).astype(F)


def around(axis, angle, azimuth):
    """float64 unit vectors `angle` away from `axis` at `azimuth` about it"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.cross(a, [0.0, 1.0, 0.0] if abs(a[1]) < 0.9 else [1.0, 0.0, 0.0])
    t /= np.linalg.norm(t)
    b = np.cross(a, t)
    return (np.cos(angle)[:, None] * a + np.sin(angle)[:, None] * (np.cos(azimuth)[:, None] * t + np.sin(azimuth)[:, None] * b))


def sky_directions(state, rng, n):
    """n // 3 uniform on the sphere, n // 3 at 1e-7 .. 1e-1 from the sun, n // 3 at 1e-7 .. 1e-3 above and below the horizon; then the sun's
    direction with its float32 neighbours, y = +0 and -0, straight up and down, the antisolar point. float32-normalised (the sun's
    direction and its neighbours are left as they are)."""
    m = n // 3
    sun = np.asarray(state, F)[48:51]
    uni = rng.normal(size=(m, 3))
    near = around(sun, 10.0 ** rng.uniform(-7, -1, m), rng.uniform(0, 2 * np.pi, m))
    az = rng.uniform(0, 2 * np.pi, m)
    y = 10.0 ** rng.uniform(-7, -3, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    hor = np.stack([np.cos(az), y, np.sin(az)], axis=1)
    nb = [sun.copy()]
    for k in range(3):
        for to in (-np.inf, np.inf):
            v = sun.copy()
            v[k] = np.nextafter(v[k], F(to))
            nb.append(v)
    flat = np.array([[1.0, 0.0, 0.0], [1.0, -0.0, 0.0], [0.6, 0.0, -0.8], [-0.6, -0.0, 0.8], [0, 1, 0], [0, -1, 0]], F)
    return np.concatenate([normalize32(uni), normalize32(near), normalize32(hor), np.array(nb, F), flat, normalize32(-sun[None].astype(np.float64))])


def sun_directions(state, rng, n):
    """n directions at angles uniform in [0, 1.3 sqrt(sin R)] from the sun (the shader's disk ends at sin^2(gamma) = sin R), n // 8 more of
    them kept only where they point below the horizon, and n // 8 on the far hemisphere (cos_gamma < 0)"""
    s = np.asarray(state, F)
    sun, reach = s[48:51], 1.3 * np.sqrt(np.sin(np.float64(s[55])))
    disk = normalize32(around(sun, rng.uniform(0, reach, n), rng.uniform(0, 2 * np.pi, n)))
    more = normalize32(around(sun, rng.uniform(0, reach, 8 * n), rng.uniform(0, 2 * np.pi, 8 * n)))
    below = more[more[:, 1] < 0][: n // 8]
    far = normalize32(around(-sun.astype(np.float64), rng.uniform(0, 1.5, n // 8), rng.uniform(0, 2 * np.pi, n // 8)))
    return np.concatenate([disk, below, far])


# ------------------------------------------------------------------ color.glsl, final_gather.rchit:68-80
def srgb_to_linear(code):
    c = np.asarray(code, np.float64) / 1023.0
    return np.where(c < float(F(0.04045)), c / float(F(12.92)), np.power(np.abs(c + float(F(0.055))) / float(F(1.055)), float(F(2.4))))


def pack_albedo(r, g, b, a=0):
    return ((np.asarray(r, np.uint32) << 22) | (np.asarray(g, np.uint32) << 12) | (np.asarray(b, np.uint32) << 2) | np.asarray(a, np.uint32)).astype(np.uint32)


def modulate_by_avg_albedo(radiance, packed):
    """(linearised albedo (n, 3), modulated colour (n, 3)), float64"""
    p = np.asarray(packed, np.uint32)
    alb = np.stack([srgb_to_linear((p >> 22) & 1023), srgb_to_linear((p >> 12) & 1023), srgb_to_linear((p >> 2) & 1023)], axis=1)
    srgb = np.asarray(radiance, F).astype(np.float64) @ ACESCG_TO_SRGB.T
    return alb, (srgb * alb) @ SRGB_TO_ACESCG.T


# ------------------------------------------------------------------ spatial_hash.glsl:105-142
def pcg(v):
    v = np.asarray(v, np.uint64) & U32
    state = (v * 747796405 + 2891336453) & U32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & U32
    return (word >> 22) ^ word


def xxhash32(p):
    h = (np.asarray(p, np.uint64) + 374761393) & U32
    h = (668265263 * (((h << 17) & U32) | (h >> 15))) & U32
    h = (2246822519 * (h ^ (h >> 15))) & U32
    h = (3266489917 * (h ^ (h >> 13))) & U32
    return h ^ (h >> 16)


def _chain(fn, pos, direction):
    pos = np.asarray(pos, np.int64).reshape(-1, 3) & U32  # the ivec3 by bit pattern
    d = np.asarray(direction, np.uint64).reshape(-1)
    h = fn(pos[:, 0].astype(np.uint64))
    h = fn((pos[:, 1].astype(np.uint64) + h) & U32)
    h = fn((pos[:, 2].astype(np.uint64) + h) & U32)
    return fn((d + h) & U32)


def key_fingerprint(pos, direction):
    return np.maximum(_chain(xxhash32, pos, direction), 1).astype(np.uint32)


def key_location(pos, direction, capacity):
    return (_chain(pcg, pos, direction) % np.asarray(capacity, np.uint64)).astype(np.uint32)


# ------------------------------------------------------------------ spatial_hash.glsl:28-93, 147-195
def _near_step(x, guard):
    return abs(x - round(x)) < guard


def logluv_encode(rgb):
    """(word, on a step)"""
    X, Y, Z = (float(v) for v in ACESCG_TO_XYZ @ np.asarray(rgb, np.float64))
    if not Y > 0:
        return 0, False
    log_y = float(F(409.6)) * (np.log2(Y) + 20.0)
    edge = _near_step(log_y, L_STEP_GUARD) and 0.5 < log_y < 16383.5
    le = int(min(max(log_y, 0.0), 16383.0))
    if le == 0:
        return 0, edge
    inv = 1.0 / (-2.0 * X + 12.0 * Y + 3.0 * (X + Y + Z))
    cu, cv = 820.0 * 4.0 * X * inv, 820.0 * 9.0 * Y * inv
    edge = edge or (_near_step(cu, UV_STEP_GUARD) and -0.5 < cu < 511.5) or (_near_step(cv, UV_STEP_GUARD) and -0.5 < cv < 511.5)
    ue, ve = int(min(max(cu, 0.0), 511.0)), int(min(max(cv, 0.0), 511.0))
    return (le << 18) | (ue << 9) | ve, edge


def logluv_decode(p):
    le = p >> 18
    if le == 0:
        return np.zeros(3)
    Y = 2.0 ** ((le + 0.5) / float(F(409.6)) - 20.0)
    u, v = (((p >> 9) & 0x1FF) + 0.5) / 820.0, ((p & 0x1FF) + 0.5) / 820.0
    inv = 1.0 / (6.0 * u - 16.0 * v + 12.0)
    x, y = 9.0 * u * inv, 4.0 * v * inv
    s = Y / y
    return np.maximum(XYZ_TO_ACESCG @ np.array([s * x, Y, s * (1.0 - x - y)]), 0.0)


def hash_insert(window, fingerprint, value, frame_index):
    """SpatialHashInsert on the three entries of one probe window, 9 words (fingerprint, radiance, last_accessed_frame | sample_count << 16
    each). Returns (the 9 words after the insert, whether the radiance word written sits on a quantisation step)."""
    w = [int(x) for x in window]
    fp, frame = int(fingerprint), int(frame_index) & 0xFFFF
    value = np.asarray(value, F).astype(np.float64)
    i_min = min_frame = 0
    for i in range(3):
        cur = w[3 * i]
        if cur == 0:
            w[3 * i] = fp  # atomicCompSwap(entry.fingerprint, 0, fingerprint)
        stamp = w[3 * i + 2] & 0xFFFF
        if i == 0 or stamp < min_frame:
            i_min, min_frame = i, stamp
        if cur == fp or cur == 0:
            rad, count = np.zeros(3), 0
            if cur == fp:
                count, rad = w[3 * i + 2] >> 16, logluv_decode(w[3 * i + 1])
            nxt = min(count, 404 - 1) + 1
            a = 1.0 / nxt
            word, edge = logluv_encode(rad * (1.0 - a) + value * a)
            w[3 * i + 1], w[3 * i + 2] = word, frame | (nxt << 16)
            return w, edge
    word, edge = logluv_encode(value)
    w[3 * i_min: 3 * i_min + 3] = [fp, word, frame | (1 << 16)]
    return w, edge


STAMPS = (0, 1, 65534, 65535, 65536, 65537)
COUNTS = (0, 1, 402, 403, 404, 65535)


def insert_cases(rng, fingerprints):
    """Rows (window[9], fingerprint, value[3], frame_index) that take every branch of the insert, per fingerprint: empty slots behind 0, 1
    or 2 strangers; the fingerprint in slot 0, 1 or 2 at every count of COUNTS; a full window of strangers with equal stamps (the
    first goes) and with distinct stamps in every order; stored stamps and frame_index over STAMPS. Values span 1e-3 .. 1e2 per
    channel, with black and a value below the LogLuv range among them."""
    import itertools
    rows = []
    stored = [s & 0xFFFF for s in STAMPS[:4]]

    def value():
        k = rng.integers(0, 12)
        if k == 0:
            return np.zeros(3, F)
        if k == 1:
            return np.full(3, 1e-9, F)
        return (10.0 ** rng.uniform(-3, 2, 3)).astype(F)

    def word():
        return logluv_encode((10.0 ** rng.uniform(-3, 2, 3)).astype(F))[0]

    def entry(fp, stamp, count=None):
        return [fp, word(), stamp | ((int(rng.choice(COUNTS)) if count is None else count) << 16)]

    for fp in (int(f) for f in fingerprints):
        strangers = [((fp ^ (0x9E3779B9 * (k + 1))) & U32) or 7 for k in range(3)]
        add = lambda w, frame: rows.append((w, fp, value(), frame))
        for frame in STAMPS:
            for before in range(3):   # an empty slot behind `before` strangers; what an empty slot's other words hold does not matter
                w = sum((entry(strangers[k], int(rng.choice(stored))) for k in range(before)), [])
                w += [0, 0, 0] if before != 1 else [0, word(), int(rng.choice(stored)) | (5 << 16)]
                w += sum((entry(strangers[k], int(rng.choice(stored))) for k in range(before + 1, 3)), [])
                add(w, frame)
            for slot in range(3):     # the fingerprint in `slot`
                for count in COUNTS:
                    w = sum((entry(strangers[k], int(rng.choice(stored))) for k in range(slot)), [])
                    w += entry(fp, int(rng.choice(stored)), count)
                    w += sum((entry(strangers[k], int(rng.choice(stored))) for k in range(slot + 1, 3)), [])
                    add(w, frame)
            for st in stored:         # strangers with equal stamps
                add(sum((entry(strangers[k], st) for k in range(3)), []), frame)
            for st in itertools.permutations(stored, 3):   # ... with distinct stamps
                add(sum((entry(strangers[k], st[k]) for k in range(3)), []), frame)
    win = np.array([r[0] for r in rows], np.uint32)
    return win, np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], F), np.array([r[3] for r in rows], np.uint32)


def logluv_fields(words):
    w = np.asarray(words, np.int64)
    return np.stack([w >> 18, (w >> 9) & 511, w & 511], axis=-1)
