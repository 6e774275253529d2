"""The source-view settings of one context across calls that resolve them differently: a region, a band, a warm-up for
another image, a refused call.  Every entry point resolves the settings into a view of its own and leaves them as the setters
did, so after each step the context must still honour exactly what was set -- against the oracle, bit for bit."""
import numpy as np
import pytest

from conftest import assert_same_mesh
from test_band import band_image
from test_gpu_band import KW, label_volume
from test_gpu_region import crop

pytestmark = pytest.mark.gpu

ARG = 1


def test_settings_survive_warm_up_and_a_refused_call(pkg, oracle):
    import torch
    shape = (40, 30, 20)
    vox, value = label_volume(shape, np.float32)
    vol = pkg.Volume(vox)
    desc = pkg.make_desc(np.float32, shape)
    kw = dict(KW, triangles=1, project=1)
    iso = value(2) + 1.0
    prm, one = pkg.make_params(iso, **kw), pkg.make_params(1, **kw)
    start, size = (3, 2, 1), (30, 20, 15)
    boxed = oracle.run(crop(vox, start, size), iso, index_start=start, **kw)
    band = (value(2), value(3), 1, 0)
    banded = oracle.run(band_image(vox, *band)[0], 1, **kw)
    assert len(boxed.cells) > 0 and len(banded.cells) > 0 and len(boxed.cells) != len(banded.cells)
    dev = torch.from_numpy(vox.reshape(-1)).cuda()
    torch.cuda.synchronize()
    ex = pkg.Extractor(0)             # a fresh context: its warm_up below runs the toy extraction
    try:
        # region set -> warm_up (a fresh context: the toy extraction runs, on its own whole volume) -> extract_host, which
        # uploads the box alone
        ex.set_region(start, size)
        ex.warm_up(pkg.make_desc(np.uint8, (64, 48, 32)), prm)
        ex.extract_host(vol, prm)
        assert_same_mesh(ex.download(), boxed)
        # ... and the region is still in force, not "already applied": the same call again, and the device route
        ex.extract_host(vol, prm)
        assert_same_mesh(ex.download(), boxed)
        # warm_up for another description on the live context: the settings are the caller's afterwards
        ex.warm_up(pkg.make_desc(np.uint8, (64, 48, 32)), prm)
        ex.extract_device(dev.data_ptr(), desc, prm)
        assert_same_mesh(ex.download(), boxed)
        # band set beside the region: refused as a pair, and a band alone with a bad bound is refused too
        ex.set_band(*band)
        with pytest.raises(pkg._abi.CuberilleError) as e:
            ex.extract_host(vol, one)
        assert e.value.code == ARG and "band" in str(e.value) and "region" in str(e.value)
        ex.clear_band()
        ex.extract_host(vol, prm)                        # the region was not dropped by the refusal
        assert_same_mesh(ex.download(), boxed)
        ex.clear_region()
        ex.set_band(value(3), value(2), 1, 0)            # lower above upper: refused at the extraction
        with pytest.raises(pkg._abi.CuberilleError) as e:
            ex.extract_host(vol, one)
        assert e.value.code == ARG and "band" in str(e.value)
        ex.set_band(*band)                               # the band after a refused call
        ex.extract_host(vol, one)
        assert_same_mesh(ex.download(), banded)
        ex.warm_up(pkg.make_desc(np.uint8, (64, 48, 32)), prm)     # (a uint8 image: the band's float values are not its)
        ex.extract_host(vol, one)
        assert_same_mesh(ex.download(), banded)
        # the region again, on the device route
        ex.clear_band()
        ex.set_region(start, size)
        ex.extract_device(dev.data_ptr(), desc, prm)
        assert_same_mesh(ex.download(), boxed)
        # everything off: the whole volume
        ex.clear_region()
        ex.extract_host(vol, prm)
        assert_same_mesh(ex.download(), oracle.run(vox, iso, **kw))
    finally:
        ex.close()
    ex = pkg.Extractor(0)             # ... and a band set before a fresh context's warm-up
    try:
        ex.set_band(*band)
        ex.warm_up(pkg.make_desc(np.uint8, (64, 48, 32)), one)
        ex.extract_device(dev.data_ptr(), desc, one)
        assert_same_mesh(ex.download(), banded)
    finally:
        ex.close()
