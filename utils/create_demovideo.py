#!/usr/bin/env python
"""Road labels for the Cityscapes demoVideo frames from a SegNet-Basic snapshot (the reference script's flags
--snapshot --out_dir --gpu --demoVideo_dir and outputs: one 0 / 1 label PNG per frame, named like the frame), and with
--out_video_fn create_movie.py's video in the same pass.  See superpixel-align_amd/demovideo.py."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    importlib.import_module('superpixel-align_amd.demovideo').demovideo_main()
