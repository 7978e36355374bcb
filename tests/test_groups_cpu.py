"""CPU suite: the f16x4 engine's launch groups (DESIGN.md "Launch groups").  The detector walks a batch in groups of pages and the encoder one in groups of
crops, as large as the widest tensor that the configuration in force hands a kernel with 32-bit buffer offsets allows inside the 2 GiB window.  The arithmetic is
pure host code (ttr_dbg_launch_groups, ttr_dbg_split_layer_check): no GPU here."""
import pytest

from tests.conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

WINDOW = (1 << 31) - 1
H, W = 1024, 768                     # the canvas of a 1024 x 768 page (h x w as the entry points take it)


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build, engine
    build.build_all()
    return engine


def test_new_symbols_are_exported_and_bound(E):
    lib = E.load()
    for name in ("ttr_dbg_launch_groups", "ttr_dbg_split_layer_check", "ttr_dbg_last_groups", "ttr_dbg_last_heat"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name
    assert E.OFFSET_WINDOW == WINDOW


def test_default_path_runs_16_page_groups(E):
    """With first_fused the 64-channel full-resolution tensor is never written: the widest is 128 channels at half resolution as pairs, 100.7 MB per page."""
    for n in (64, 32, 16):
        gp, _, per_page, _ = E.launch_groups(H, W, n, 1)
        assert gp == 16 and per_page == (H // 2) * (W // 2) * 128 * 4 == 100663296
        assert gp * per_page == 1610612736 <= WINDOW


def test_batches_that_16_does_not_divide(E):
    assert E.launch_groups(H, W, 24, 1)[0] == 8          # 8 + 8 + 8, not 16 + 8
    assert E.launch_groups(H, W, 40, 1)[0] == 8
    assert E.launch_groups(H, W, 20, 1)[0] == 16         # as before: 16 + 4
    assert E.launch_groups(H, W, 5, 1)[0] == 16          # (one group of 5: the caller takes min(group, n))
    assert E.launch_groups(H, W, 64, 1, craft_group=8)[0] == 8     # the A/B key: the schedule of before
    assert E.launch_groups(H, W, 64, 1, craft_group=32)[0] == 16   # 21 fit; evened
    assert E.launch_groups(H, W, 63, 1, craft_group=32)[0] == 21   # what the window allows, and never more
    assert E.launch_groups(H, W, 16, 1, craft_group=5)[0] == 5


def test_other_configurations_keep_their_figure(E):
    """Without first_fused the 64-channel tensor at full resolution exists: 201 MB per page as pairs, 10 pages, evened to 8.  As triples (craft_products = 4: six
    bytes per value, and no fused first pair) it is 302 MB: 7 pages fit and 8 would not (8 x 301 989 888 = 2 415 919 104 > 2^31 - 1), so the group stays 7, the
    figure of before."""
    gp, _, per_page, _ = E.launch_groups(H, W, 64, 1, first_fused=0)
    assert (gp, per_page) == (8, H * W * 64 * 4)
    assert E.launch_groups(H, W, 30, 1, first_fused=0)[0] == 10
    for ff in (0, 1):
        gp, _, per_page, _ = E.launch_groups(H, W, 64, 1, first_fused=ff, craft_products=4)
        assert (gp, per_page) == (7, H * W * 64 * 6)
        assert 8 * per_page > WINDOW
    # the commuted up-convolutions change which tensors exist, not the widest
    assert E.launch_groups(H, W, 64, 1, up_commute=0)[:3:2] == (16, 100663296)


def test_a_large_page_gets_what_the_window_allows(E):
    gp, _, per_page, _ = E.launch_groups(2048, 1536, 64, 1)      # a 2048 x 1536 page on a canvas of its own size
    assert per_page == 4 * 100663296 and gp == 5 == WINDOW // per_page
    assert (gp + 1) * per_page > WINDOW
    gp, _, per_page, _ = E.launch_groups(2048, 1536, 64, 1, first_fused=0)
    assert gp == 2 == WINDOW // per_page
    assert E.launch_groups(256, 192, 24, 1)[0] == 8 and E.launch_groups(256, 192, 20, 1)[0] == 16    # small pages: the key alone


ONE = 4096                           # enc_chunk large enough to lift the default cap of 1820 crops: the window alone decides


def test_encoder_groups(E):
    """The MLP hidden as pairs is 1536 x 4 bytes per row, 128 rows per crop: 2730 crops fit.  With the key lifted 2560 crops are one group, 2731 two even ones.
    The DEFAULT stays the cap of before (1820: 2560 crops = 1280 + 1280): one group did not pass its A/B (profiles/groups.md)."""
    _, ge, _, per_crop = E.launch_groups(H, W, 1, 2560, enc_chunk=ONE)
    assert ge == 2560 and per_crop == 128 * 1536 * 4 and 2560 * per_crop == 2013265920 <= WINDOW
    assert E.launch_groups(H, W, 1, 2730, enc_chunk=ONE)[1] == 2730
    assert E.launch_groups(H, W, 1, 2731, enc_chunk=ONE)[1] == 1366               # 1366 + 1365
    assert E.launch_groups(H, W, 1, 2600, enc_chunk=ONE)[1] == 2600
    assert E.launch_groups(H, W, 1, 4096, enc_chunk=ONE)[1] == 2048
    assert E.launch_groups(H, W, 1, 2560, enc_chunk=ONE, sp_hidden16=2)[1] == 2560    # another layout of the same bytes
    assert E.launch_groups(H, W, 1, 40)[1] == 40
    assert E.launch_groups(H, W, 1, 1820)[1] == 1820
    assert E.launch_groups(H, W, 1, 2560)[1] == 1280                              # the default: as before
    assert E.launch_groups(H, W, 1, 2560, enc_chunk=1280)[1] == 1280
    assert E.launch_groups(H, W, 1, 2560, enc_chunk=640)[1] == 640
    assert E.launch_groups(H, W, 1, 4096)[1] == 1366                              # 3 groups, as before


def test_encoder_configurations_that_keep_their_figure(E):
    """The hidden as triples: 1820 crops, as before, whatever the key says.  The unfused qkv path writes qkv as triples, 3 x 384 x 6 bytes per row - wider than a
    hidden of pairs - and stays under 2560 crops."""
    for chunk in (0, ONE):
        _, ge, _, per_crop = E.launch_groups(H, W, 1, 2560, enc_chunk=chunk, enc_fc2_pairs=0)
        assert per_crop == 128 * 1536 * 6 and WINDOW // per_crop == 1820 and ge == 1280
        assert E.launch_groups(H, W, 1, 1820, enc_chunk=chunk, enc_fc2_pairs=0)[1] == 1820
        assert E.launch_groups(H, W, 1, 1821, enc_chunk=chunk, enc_fc2_pairs=0)[1] == 911
    for kw in (dict(qkv_attn_split=0), dict(enc_ln_pairs=0)):         # (the fused launch needs LayerNorm pairs)
        _, ge, _, per_crop = E.launch_groups(H, W, 1, 2560, enc_chunk=ONE, **kw)
        assert per_crop == 128 * 3 * 384 * 6 and WINDOW // per_crop == 2427 and ge == 1280
        assert E.launch_groups(H, W, 1, 2427, enc_chunk=ONE, **kw)[1] == 2427
        assert E.launch_groups(H, W, 1, 2560, **kw)[1] == 1280
    assert E.launch_groups(H, W, 1, 2560, enc_chunk=ONE, qkv_attn_split=0, enc_fc2_pairs=0)[1] == 1280   # the hidden as triples leads again


def test_no_group_leaves_the_window(E):
    for (h, w) in ((768, 1024), (1536, 2048), (192, 256), (2560, 2560), (32, 32)):
        for n in (1, 7, 8, 16, 24, 32, 63, 64):
            for cg in (1, 8, 16, 32):
                for ff in (0, 1):
                    for prod in (3, 4):
                        for uc in (0, 1):
                            gp, _, per_page, _ = E.launch_groups(h, w, n, 1, craft_group=cg, first_fused=ff, craft_products=prod, up_commute=uc)
                            assert 1 <= gp <= cg and (gp * per_page <= WINDOW or gp == 1), (h, w, n, cg, ff, prod, uc, gp)
    for N in (1, 40, 1280, 1820, 1821, 2427, 2428, 2560, 2600, 2730, 2731, 4096):
        for chunk in (0, 640, 1280, 5000):
            for pairs in (0, 1):
                for fused in (0, 1):
                    for lnp in (0, 1):
                        _, ge, _, per_crop = E.launch_groups(H, W, 1, N, enc_chunk=chunk, enc_fc2_pairs=pairs, qkv_attn_split=fused, enc_ln_pairs=lnp)
                        assert 1 <= ge <= N and ge * per_crop <= WINDOW and ge <= (chunk or 1820), (N, chunk, pairs, fused, lnp, ge)
                        groups = -(-N // ge)
                        assert ge == -(-N // groups)                # even groups


def test_bad_arguments_are_refused(E):
    for bad in ((H + 1, W, 1, 1), (0, W, 1, 1), (H, W, 0, 1), (H, W, 1, 0)):
        with pytest.raises(E.EngineError):
            E.launch_groups(*bad)


def test_launchers_refuse_a_tensor_past_the_window(E):
    """The shape checks of the layer launchers themselves, at the sizes of the default path: 16 pages of 1024 x 768 pass every one; 22 pages put slice1.7's OUTPUT
    (128 channels at half resolution as pairs: 2.2 GB) past the window while its input (64 channels: 1.1 GB) is inside it, and the launcher refuses to make it."""
    h1, w1 = H // 2, W // 2
    for B in (8, 16):
        assert E.split_layer_check("conv3p", B, h1, w1, 64, 128) is None                       # slice1.7
        assert E.split_layer_check("conv3p", B, h1, w1, 128, 128, pooled=True) is None         # slice1.10 (+ pool)
        assert E.split_layer_check("conv3p", B, H // 4, W // 4, 256, 256) is None              # slice2.17
        assert E.split_layer_check("gemm2", B, H // 16, W // 16, 1024, 1024, ks=1) is None     # slice5.2
        assert E.split_layer_check("gemm2", B, H // 8, W // 8, 512, 256, ks=1) is None         # upconv2.0, skip half
    # the fused first pair reads the u8 canvas (3 bytes per pixel) and never forms its 64-channel input; the unfused slice1.3 would read 3.2 GB at 16 pages
    assert E.split_layer_check("conv3p_first", 16, H, W, 64, 64, pooled=True) is None
    assert "too large" in E.split_layer_check("conv3p", 16, H, W, 64, 64, pooled=True)
    assert "output too large" in E.split_layer_check("conv3p", 22, h1, w1, 64, 128)
    assert "too large" in E.split_layer_check("conv3p", 22, h1, w1, 128, 128)                  # its consumer: the input is past the window
    assert "output too large" in E.split_layer_check("gemm2", 22, h1, w1, 64, 128, ks=1)
    # the encoder's linears at 2560 crops (M = 327 680 rows): fc1 writes the hidden as pairs (2 013 265 920 B), fc2 reads it; as triples neither fits
    M = 2560 * 128
    assert E.split_layer_check("gemm2", 1, 1, M, 384, 1536, ks=1, out_planes=2) is None
    assert E.split_layer_check("gemm2", 1, 1, M, 1536, 384, ks=1, out_planes=0) is None
    assert "output too large" in E.split_layer_check("gemm2", 1, 1, M, 384, 1536, ks=1, out_planes=3)
    assert "too large" in E.split_layer_check("gemm2", 1, 1, M, 1536, 384, ks=1, products=4, out_planes=0)
    assert "output too large" in E.split_layer_check("gemm2", 1, 1, 2731 * 128, 384, 1536, ks=1, out_planes=2)
