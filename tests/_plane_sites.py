"""Host-side enumeration of the convolution launches that read prepared weight planes ("plane sites") in the five zoo models, and
the library's answers about each of them.  Shared by tests/test_plane_sites_gpu.py and scripts/plan_table.py.

A site is what `Node.plane_sites(rt, batch)` yields (Conv2D, the pointwise half of SeparableConv2D, Conv2DTranspose; the call is
`_Runtime.ensure_planes`): the forward-convolution descriptor, the direction (dgrad = 1: input gradient / Conv2DTranspose forward),
whether it is the fp32 softmax head of a bf16 model, and where the layer's kernel lies in the model's weight arena.  Nothing is run
forward and no device memory is touched here: only shapes and weight offsets are needed.  The stand-in runtime below answers
`up2_on` with False, so the forward of the convolution behind a fused UpSampling2D(2) is listed as well: the product takes it
through the prepared planes whenever the fused kernels are off (arithmetic modes 0 and 2, SG_UP2_FUSE=0).
"""
import collections
import ctypes as C

MODELS = ("v3plus", "bam", "scse", "res34", "hrnet")
POLICIES = ("float32", "mixed_bfloat16")
# (input size, batch sizes, backward sites too): the models' default 512 x 512 as compiled for training, and bench config 5
# (1024 x 1024, batch 8) forward only
GEOMETRIES = ((512, (1, 2, 8, 16), True), (1024, (8,), False))

Site = collections.namedtuple("Site", "model size batch policy tag desc dgrad head convt w_off w_shape")
Group = collections.namedtuple("Group", "model size batch policy n_train sites")


def desc_fields():
    from building_detection_amd import _lib
    return tuple(n for n, _ in _lib.ConvDesc._fields_)


def build_model(name, size, policy):
    from building_detection_amd import mixed_precision as MP, zoo
    MP.set_global_policy(policy)
    try:
        if name in ("v3plus", "bam"):
            return zoo.BUILDERS[name]((size, size, 3), 2, aspp_pool=size // 16)
        return zoo.BUILDERS[name]((size, size, 3))
    finally:
        MP.set_global_policy("float32")


class _SiteRuntime:
    """What `plane_sites` asks of a runtime, without one: descriptors (Engine.conv_desc is static), `needs_grad` and `up2_on`."""

    def __init__(self, model):
        from building_detection_amd.ops import Engine
        self.model = model
        self.eng = Engine   # only the static conv_desc is used

    def needs_grad(self, sym):
        from building_detection_amd.runtime import _Runtime
        return _Runtime.needs_grad(self, sym)

    def up2_on(self, up_node):
        return False


def enumerate_groups(models=MODELS, policies=POLICIES, geometries=GEOMETRIES):
    """One Group per (model, input size, batch, policy) with every site of the model in node order (the job table the runtime
    would build for that batch), trainable kernels only, backward sites where the geometry has them."""
    fields = desc_fields()
    groups = []
    for name in models:
        for size, batches, bwd in geometries:
            for policy in policies:
                model = build_model(name, size, policy)
                rt = _SiteRuntime(model)
                for batch in batches:
                    sites = []
                    for n in model.nodes:
                        fn = getattr(n, "plane_sites", None)
                        if fn is None:
                            continue
                        for tag, wspec, d, dgrad, phase, head in fn(rt, int(batch)):
                            if (phase == "bwd" and not bwd) or not wspec.trainable:
                                continue
                            sites.append(Site(name, size, int(batch), policy, tag, tuple(int(getattr(d, f)) for f in fields), int(dgrad),
                                              bool(head), n.op == "conv2d_transpose", int(wspec.offset), tuple(wspec.shape)))
                    groups.append(Group(name, size, int(batch), policy, int(model._n_train), sites))
    return groups


def site_key(s):
    """De-duplication key: the descriptor fields, the direction, the head flag and the storage type."""
    return (s.desc, s.dgrad, s.head, s.policy)


def unique_sites(groups):
    """-> ({key: Site}, {key: index of the first group that has it}).  A Conv2DTranspose forward that shares its descriptor with a
    plain input gradient keeps the transposed layer's epilogue runs (convt is OR-ed)."""
    first, owner = collections.OrderedDict(), {}
    for gi, g in enumerate(groups):
        for s in g.sites:
            k = site_key(s)
            if k not in first:
                first[k] = s
                owner[k] = gi
            elif s.convt and not first[k].convt:
                first[k] = first[k]._replace(convt=True)
    return first, owner


def make_desc(s):
    from building_detection_amd import _lib
    return _lib.ConvDesc(*s.desc)


def abi_dtype(s):
    from building_detection_amd import _lib
    if s.policy == "float32":
        return _lib.SG_F32
    return _lib.SG_BF16 | (_lib.SG_HEAD_F32 if s.head else 0)


def planes_job(engine, s):
    """sg_conv2d_planes_job of site `s` under the CURRENT arithmetic mode -> (job, bytes)."""
    from building_detection_amd import _lib
    d = make_desc(s)
    job, nbytes = _lib.PlanesJob(), C.c_size_t(0)
    _lib.check(engine.lib.sg_conv2d_planes_job(engine.h, abi_dtype(s), C.byref(d), s.dgrad, C.byref(job), C.byref(nbytes)),
               "sg_conv2d_planes_job")
    return job, int(nbytes.value)


def planes_in(engine, s):
    """sg_conv2d_caps' planes_in: the launch reads its activation as split_planes' planes (fp32 storage, mode 1)."""
    d = make_desc(s)
    return int(engine.conv2d_caps(d, s.dgrad).planes_in) if s.policy == "float32" else 0


def ws_query(engine, s):
    d = make_desc(s)
    fn = engine.lib.sg_conv2d_dgrad_ws_bytes if s.dgrad else engine.lib.sg_conv2d_fwd_ws_bytes
    return int(fn(C.byref(d)))


def macs(s):
    f = dict(zip(desc_fields(), s.desc))
    return f["N"] * f["Ho"] * f["Wo"] * f["Cout"] * f["KH"] * f["KW"] * f["Cin"]


def modes_of(policy):
    """Arithmetic modes a storage type is run under: fp32 storage in all three, bf16 storage in the default one only."""
    return (0, 1, 2) if policy == "float32" else (None,)


class mode_set:
    """`with mode_set(engine, mode):` runs the block under arithmetic mode `mode` (None: leave it) and restores the previous one.
    The switch is process-wide and every job table depends on it: build the tables inside the block."""

    def __init__(self, engine, mode):
        self.lib, self.mode, self.prev = engine.lib, mode, None

    def __enter__(self):
        if self.mode is not None:
            self.prev = self.lib.sg_set_conv_x6(int(self.mode))
        return self

    def __exit__(self, *exc):
        if self.mode is not None:
            self.lib.sg_set_conv_x6(self.prev)
        return False


JOB_FIELDS = ("kind", "npl", "kd", "K", "Kpad", "N", "Npad", "Ck", "Ckp", "nblocks")
Info = collections.namedtuple("Info", JOB_FIELDS + ("bytes", "ws", "pin", "cls"))


def survey(engine, uniq):
    """{(key, mode): Info} - the planes job, the workspace query and the planes-in answer of every unique site under every
    arithmetic mode its storage type is run in."""
    out = collections.OrderedDict()
    for mode in (0, 1, 2, None):
        with mode_set(engine, mode):
            for k, s in uniq.items():
                if mode not in modes_of(s.policy):
                    continue
                job, nbytes = planes_job(engine, s)
                pin = planes_in(engine, s)
                out[(k, mode)] = Info(*(int(getattr(job, f)) for f in JOB_FIELDS), nbytes, ws_query(engine, s), pin,
                                      plan_class(s, mode, job, pin))
    return out


def representatives(uniq, info):
    """{class: (key, mode)}: in every plan class the site with the fewest multiply-adds (the first of them in enumeration order)."""
    reps = collections.OrderedDict()
    for (k, mode), i in info.items():
        cur = reps.get(i.cls)
        if cur is None or macs(uniq[k]) < macs(uniq[cur[0]]):
            reps[i.cls] = (k, mode)
    return reps


def plan_class(s, mode, job, pin):
    """What the ABI reveals of the plan: the grouping of the oracle check (one representative per class)."""
    f = dict(zip(desc_fields(), s.desc))
    return (s.policy, mode, s.dgrad, int(job.kind), int(job.npl), int(job.kd), bool(job.Ckp != job.Ck),
            bool(job.Npad != job.N), int(pin), f["stride"], f["dilation"] > 1, s.head)


def describe(s):
    f = dict(zip(desc_fields(), s.desc))
    return (f"{s.model}/{s.size}/b{s.batch}/{'bf16' if s.policy != 'float32' else 'f32'} {'dgrad' if s.dgrad else 'fwd'}"
            f"{'(convT)' if s.convt else ''}{'(head)' if s.head else ''} {f['N']}x{f['H']}x{f['W']}x{f['Cin']}->{f['Cout']} "
            f"k{f['KH']} s{f['stride']} d{f['dilation']}")
