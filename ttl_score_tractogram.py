#!/usr/bin/env python3
"""Console entry point: tracktolearn_amd.runners.ttl_score_tractogram.main
(score a .trk / .tck with the Tractometer validator)."""
from tracktolearn_amd.runners.ttl_score_tractogram import main

if __name__ == '__main__':
    main()
