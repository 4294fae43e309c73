"""The comparison of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/conv_tile_outputs_compare.txt (the sibling of
tools/conv_wdma_outputs_compare.py, whose verdicts it prints):

    python tools/conv_tile_outputs_compare.py PARENT_A PARENT_B NEW > profiles/conv_tile_outputs_compare.txt

PARENT_* ran on the parent commit's build (4 x 32 tiles everywhere), NEW on this one with the planned tile geometries, same arguments,
same routing.  Which pixels a workgroup takes changes no operand and no order of additions of a map's element; the bias gradients are
float64 sums rounded once.  Exit status 1 if an array differs."""
import sys

from conv_wdma_outputs_compare import main

if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:4]))
