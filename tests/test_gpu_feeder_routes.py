"""GPU: every FrameFeeder route on ONE folder -- jpeg in {host, device, device_entropy, device_sync} x png in {host, device} -- against
the host/host route and frame_io.imread: frames byte for byte, batch boundaries, and the frames each entropy route leaves to the host
decoder.  The folder holds every kind of file a stage can be handed, a batch that mixes them, and a ragged last batch."""
import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
import jpeg_entropy_cases as E
import png_in_cases as P
from semantic_depth_amd import frame_io, outputs

pytestmark = pytest.mark.gpu

H, W, BATCH = 48, 80, 4
PROGRESSIVE, NO_DRI = 5, (0, 2, 7, 8)                      # indices in the folder below
# (global frame index, why) of the frames that take the host decoder: without restart intervals nothing is eligible on the entropy route
ENTROPY_FALLBACK = [(i, "ineligible") for i in sorted(NO_DRI + (PROGRESSIVE,))]
SYNC_FALLBACK = [(PROGRESSIVE, "ineligible")]


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """nine files of 48 x 80 after the orientation.  Batch 0: 4:4:4 without DRI, a palette PNG next to it, 4:2:2 without DRI, a Pillow
    restart file; batch 1: the project's encoder, a progressive file, an RGB PNG, EXIF orientation 6 (stored 80 x 48); batch 2: 4:2:0"""
    PILImage = pytest.importorskip("PIL.Image")
    import io
    tmp = tmp_path_factory.mktemp("routes")
    rng = np.random.default_rng(77)

    def pil(img, **kw):
        b = io.BytesIO()
        PILImage.fromarray(img).save(b, "JPEG", quality=88, **kw)
        return b.getvalue()
    pal = rng.integers(0, 256, (40, 3), dtype=np.uint8)
    files = [
        ("f0_444.jpg", pil(J._img(rng, H, W), subsampling=0)),
        ("f1_palette.png", P.make_png(rng.integers(0, 40, (H, W, 1), dtype=np.uint8), 3, rng.integers(0, 5, H), palette=pal)),
        ("f2_422.jpg", pil(J._img(rng, H, W), subsampling=1)),
        ("f3_restart.jpg", pil(J._img(rng, H, W), subsampling=2, restart_marker_rows=1)),
        ("f4_own.jpg", E.own_jpeg(J._img(rng, H, W), 85)),
        ("f5_progressive.jpg", pil(J._img(rng, H, W), progressive=True)),
        ("f6_rgb.png", None),
        ("f7_exif6.jpg", J.with_orientation(pil(J._img(rng, W, H), subsampling=2), 6)),
        ("f8_420.jpg", pil(J._img(rng, H, W), subsampling=2)),
    ]
    paths = []
    for name, data in files:
        p = str(tmp / name)
        if data is None:
            outputs.write_png(p, J._img(rng, H, W))
        else:
            open(p, "wb").write(data)
        paths.append(p)
    return paths


def _passes(feeder):
    got, los = [], []
    for dev, lo in feeder:
        assert dev.is_cuda and dev.is_contiguous()
        got.append(dev.cpu().numpy())
        los.append(lo)
    return got, los, list(feeder.entropy_fallback), list(feeder.sync_fallback)


def _feeder(paths, eng, jpeg, png):
    kw = dict(engine=eng) if (jpeg, png) != ("host", "host") else {}
    return frame_io.FrameFeeder(paths, batch=BATCH, device="cuda", workers=3, jpeg=jpeg, png=png, **kw)


@pytest.fixture(scope="module")
def host_route(eng, folder):
    with _feeder(folder, eng, "host", "host") as feeder:
        got, los, ent, syn = _passes(feeder)
    assert los == [0, 4, 8] and [g.shape for g in got] == [(4, H, W, 3), (4, H, W, 3), (1, H, W, 3)] and ent == syn == []
    for frame, p in zip(np.concatenate(got), folder):
        assert np.array_equal(frame, frame_io.imread(p)), p
    return got, los


@pytest.mark.parametrize("png", ["host", "device"])
@pytest.mark.parametrize("jpeg", ["host", "device", "device_entropy", "device_sync"])
def test_every_route_feeds_the_frames_of_the_host_route(eng, folder, host_route, jpeg, png):
    host, los_h = host_route
    with _feeder(folder, eng, jpeg, png) as feeder:
        got, los, ent, syn = _passes(feeder)
    assert los == los_h and [g.shape for g in got] == [g.shape for g in host]
    for k, (a, b) in enumerate(zip(host, got)):
        assert np.array_equal(a, b), (k, np.argwhere((a != b).any((1, 2, 3))).ravel())
    for frame, p in zip(np.concatenate(got), folder):
        assert np.array_equal(frame, frame_io.imread(p)), p
    assert ent == (ENTROPY_FALLBACK if jpeg == "device_entropy" else [])
    assert syn == (SYNC_FALLBACK if jpeg == "device_sync" else [])


@pytest.mark.parametrize("jpeg,want", [("device_entropy", ENTROPY_FALLBACK), ("device_sync", SYNC_FALLBACK)])
def test_a_second_pass_of_one_feeder_equals_the_first(eng, folder, host_route, jpeg, want):
    with _feeder(folder, eng, jpeg, "device") as feeder:
        first = _passes(feeder)
        second = _passes(feeder)
    assert first[1:] == second[1:] and all(np.array_equal(a, b) for a, b in zip(first[0], second[0]))
    assert all(np.array_equal(a, b) for a, b in zip(first[0], host_route[0]))
    assert (second[2], second[3]) == ((want, []) if jpeg == "device_entropy" else ([], want))      # the lists do not accumulate
