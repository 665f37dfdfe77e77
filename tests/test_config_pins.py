"""easyrec_amd/utils/config_util.py:get_configs_from_pipeline_file against the REFERENCE'S OWN (utils/config_util.py:46-136,
executed by tests/golden/make_config_vectors.py): the loaded message - with `shared_names` and `name[1-13]` ranges
expanded - in full text for three embedded inputs.  The digests the fixture holds for every config the reference ships
are checked where a config of this repository restates one (tests/test_proto_config.py)."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'config_vectors.json')) as f:
  FIX = json.load(f)


@pytest.mark.parametrize('tag', sorted(FIX['embedded']))
def test_embedded_configs_expand_as_the_reference_expands_them(tag, tmp_path):
  from google.protobuf import text_format

  from easyrec_amd.utils import config_util
  path = tmp_path / ('%s.config' % tag)
  path.write_text(FIX['embedded'][tag]['input'])
  got = config_util.get_configs_from_pipeline_file(str(path))
  assert text_format.MessageToString(got) == FIX['embedded'][tag]['loaded']
