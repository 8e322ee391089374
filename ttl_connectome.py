#!/usr/bin/env python3
"""Console entry point: tracktolearn_amd.runners.ttl_connectome.main
(the structural connectome of a .trk / .tck on a label image)."""
from tracktolearn_amd.runners.ttl_connectome import main

if __name__ == '__main__':
    main()
