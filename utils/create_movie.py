#!/usr/bin/env python
"""The demo video from the label PNGs of create_demovideo.py (the reference script's flags --pred_label_dir --img_dir
--out_video_fn and defaults): the road colour blended into every frame, an MJPG .avi at 30 fps.  No GPU is used.  See
superpixel-align_amd/demovideo.py."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    importlib.import_module('superpixel-align_amd.demovideo').movie_main()
