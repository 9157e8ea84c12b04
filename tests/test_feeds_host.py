"""feeds.feed_kind: the forcing path of an offline run, chosen from the
provider and the driver's arguments alone (no device work), over stub
providers -- plain objects with the methods the choice asks for."""
import pytest

from noahmp_amd import feeds


class Callable12:
    """A provider of the 12 fields (forcing(step, t)), nothing else."""
    def __call__(self, step, t):
        raise AssertionError("feed_kind reads no forcing")


class Files(Callable12):
    """What ncio.LdasinForcing offers on the model grid, host-side only."""
    def raw(self, step, t, out=None): ...
    def block(self, t, out=None): ...
    def variables(self, t): ...
    def geo(self): ...


class FilesIngest(Files):
    def grid_raw(self, t, out=None): ...
    plan = None


class FilesCoarse(FilesIngest):
    plan = object()   # a regrid plan
    def dz(self): ...


class OnDevice:
    on_device = True


@pytest.mark.parametrize("forcing", [None, Callable12(), lambda step, t: None])
@pytest.mark.parametrize("ldasin_upload", [True, False])
@pytest.mark.parametrize("cosz", ["device", "host"])
@pytest.mark.parametrize("ingest", [True, False])
def test_twelve_field_providers_take_the_host_feed(forcing, ldasin_upload, cosz, ingest):
    assert feeds.feed_kind(forcing, ldasin_upload, cosz, ingest) == "host"


@pytest.mark.parametrize("provider", [Files(), FilesIngest(), FilesCoarse()])
@pytest.mark.parametrize("cosz", ["device", "host"])
@pytest.mark.parametrize("ingest", [True, False])
def test_files_without_ldasin_upload_take_the_host_feed(provider, cosz, ingest):
    assert feeds.feed_kind(provider, False, cosz, ingest) == "host"


@pytest.mark.parametrize("forcing", ["device", OnDevice()])
@pytest.mark.parametrize("ldasin_upload", [True, False])
@pytest.mark.parametrize("cosz", ["device", "host"])
def test_device_forcing(forcing, ldasin_upload, cosz):
    assert feeds.feed_kind(forcing, ldasin_upload, cosz, True) == "device-synth"


@pytest.mark.parametrize("provider", [Files(), FilesIngest(), FilesCoarse()])
@pytest.mark.parametrize("ingest", [True, False])
def test_host_cosz_uploads_every_step(provider, ingest):
    assert feeds.feed_kind(provider, True, "host", ingest) == "ldasin-step"


@pytest.mark.parametrize("provider, ingest, kind", [
    (Files(), True, "ldasin-block"),          # no grid_raw: nothing to ingest
    (Files(), False, "ldasin-block"),
    (FilesIngest(), False, "ldasin-block"),   # grid_raw, but ingest=False
    (FilesCoarse(), False, "ldasin-block"),
    (FilesIngest(), True, "ldasin-ingest"),
    (FilesCoarse(), True, "ldasin-regrid"),   # a provider with a plan
])
def test_resident_blocks(provider, ingest, kind):
    assert feeds.feed_kind(provider, True, "device", ingest) == kind
    assert feeds.feed_kind(provider, ldasin_upload=True, cosz="device", ingest=ingest,
                           downscale=False) == kind


def test_defaults_are_the_drivers():
    assert feeds.feed_kind(FilesIngest()) == "ldasin-ingest"
    assert feeds.feed_kind(None) == "host"


@pytest.mark.parametrize("ingest, kind", [(True, "ldasin-regrid"), (False, "ldasin-block")])
def test_downscale_keeps_the_kind(ingest, kind):
    assert feeds.feed_kind(FilesCoarse(), True, "device", ingest, downscale=True) == kind


@pytest.mark.parametrize("provider, ldasin_upload, cosz", [
    (FilesCoarse(), True, "host"), (FilesCoarse(), False, "device"), (Callable12(), True, "device"),
    (None, True, "device"), ("device", True, "device")])
def test_downscale_without_resident_blocks_is_refused(provider, ldasin_upload, cosz):
    with pytest.raises(ValueError, match="downscale needs LDASIN files uploaded as resident"):
        feeds.feed_kind(provider, ldasin_upload, cosz, True, downscale=True)


@pytest.mark.parametrize("provider", [Files(), FilesIngest()])
def test_downscale_without_a_forcing_grid_is_refused(provider):
    with pytest.raises(ValueError, match="downscale needs LDASIN files on a forcing grid"):
        feeds.feed_kind(provider, True, "device", True, downscale=True)


@pytest.mark.parametrize("provider", [None, Files(), "device"])
def test_bad_cosz_is_refused(provider):
    with pytest.raises(ValueError, match="cosz must be 'device' or 'host', not 'gpu'"):
        feeds.feed_kind(provider, True, "gpu", True)
    with pytest.raises(ValueError, match="cosz must be"):   # before the downscale checks
        feeds.feed_kind(provider, True, "gpu", True, downscale=True)
