"""CPU: which products gemm_plan (csrc/gemm.hip) gives to the weight-resident split-bf16 form under the default knobs, asked through
bbbp_gemm_kernel_form.  Without a GPU the plan assumes 256 CUs, the MI355X's count."""
from bbbp_amd import _lib

DIRECT, B3, RESIDENT = 0, 2, 6


def test_default_plan_gives_the_resident_form_the_image_fc_input_gradient_only():
    form = _lib.lib().bbbp_gemm_kernel_form
    # dpool2[B][65536] = dcomb[:, 128:256] W[128][65536] at the batch sizes with at least two row tiles
    for B in (256, 300, 512, 4096):
        assert form(0, 0, B, 65536, 128, 1) == RESIDENT
    assert form(0, 0, 512, 256 * 128, 96, 1) == RESIDENT          # exactly one column block per CU, three k stages
    # one row tile; fewer column blocks than CUs; K past four stages or not whole stages; ragged N; a batch; the other layouts
    assert form(0, 0, 128, 65536, 128, 1) == B3
    assert form(0, 0, 512, 255 * 128, 128, 1) == B3
    assert form(0, 0, 512, 65536, 160, 1) == B3
    assert form(0, 0, 512, 65536, 100, 1) == B3
    assert form(0, 0, 512, 65536 + 4, 128, 1) == B3
    assert form(0, 0, 512, 65536, 128, 2) == B3
    assert form(0, 1, 512, 65536, 128, 1) == B3
    assert form(1, 0, 512, 65536, 128, 1) == B3
    assert form(0, 0, 384, 384, 128, 1) == DIRECT                 # the GPU test's shapes stay where they were unless the knob's bit 1 is set
    assert form(1, 1, 8, 8, 8, 1) == -1 and form(0, 0, 0, 8, 8, 1) == -1
